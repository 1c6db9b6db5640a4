/* tiff_window.c -- a window of an open TIFF file: its pixels through the host decoders (gcn10_tiff_read_window[_mt]),
 * or the plan of its chunks for the GPU decoders (gcn10_tiff_plan_window).  Both walk the chunks the window touches
 * and clip each against it with the same two functions, so the two paths cannot disagree about which pixel of which
 * chunk goes where.  (The module as a whole: tiff_internal.h.)
 */
#include "tiff_internal.h"

#include <stdatomic.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

struct window {
    int xoff, yoff, xcount, ycount;
};

/* 0 = the window has pixels and lies inside the raster; -1 = it does not (err is set) */
static int window_in_raster(const struct gcn10_tiff *t, const struct window *w, char *err, size_t errcap)
{
    if (w->xoff < 0 || w->yoff < 0 || w->xcount <= 0 || w->ycount <= 0 ||
        (uint64_t)w->xoff + (uint64_t)w->xcount > t->width || (uint64_t)w->yoff + (uint64_t)w->ycount > t->height) {
        snprintf(err, errcap, "window %d,%d %dx%d outside raster %ux%u", w->xoff, w->yoff, w->xcount, w->ycount,
                 t->width, t->height);
        return -1;
    }
    return 0;
}

/* the chunks a window (inside the raster) touches: columns cx0 .. cx1 of rows cy0 .. cy1 of the chunk grid */
struct chunk_range {
    uint32_t cx0, cx1, cy0, cy1;
};

static struct chunk_range chunks_of_window(const struct gcn10_tiff *t, const struct window *w)
{
    return (struct chunk_range){ (uint32_t)w->xoff / t->cw, (uint32_t)(w->xoff + w->xcount - 1) / t->cw,
                                 (uint32_t)w->yoff / t->ch, (uint32_t)(w->yoff + w->ycount - 1) / t->ch };
}

/* chunk (cx, cy) against a window */
struct chunk_clip {
    uint64_t idx;               /* of the chunk in the directory's arrays */
    uint32_t x_lo, y_lo;        /* the chunk's first pixel, in the raster */
    uint32_t rows;              /* rows the chunk holds: a tile always ch, the last strip what is left of the raster */
    uint32_t xs, xe, ys, ye;    /* the window's part of the chunk, [xs, xe) x [ys, ye) in the raster */
};

/* false = the window has no pixel in the chunk */
static bool clip_chunk(const struct gcn10_tiff *t, uint32_t cx, uint32_t cy, const struct window *w,
                       struct chunk_clip *c)
{
    const uint32_t x0 = (uint32_t)w->xoff, x1 = (uint32_t)(w->xoff + w->xcount);
    const uint32_t y0 = (uint32_t)w->yoff, y1 = (uint32_t)(w->yoff + w->ycount);

    c->idx = (uint64_t)cy * t->across + cx;
    c->x_lo = cx * t->cw;
    c->y_lo = cy * t->ch;
    c->rows = t->tiled || c->y_lo + t->ch <= t->height ? t->ch : t->height - c->y_lo;
    c->xs = x0 > c->x_lo ? x0 : c->x_lo;
    c->xe = x1 < c->x_lo + t->cw ? x1 : c->x_lo + t->cw;
    c->ys = y0 > c->y_lo ? y0 : c->y_lo;
    c->ye = y1 < c->y_lo + c->rows ? y1 : c->y_lo + c->rows;
    return c->xs < c->xe && c->ys < c->ye;
}

/* one chunk (tile or strip) of a window read: decode and copy the overlap */
struct chunk_job {
    struct gcn10_tiff *t;
    uint32_t cx, cy;
    struct window w;
    uint8_t *dst;
    size_t dst_stride;
    struct gcn10_job_group *group;  /* the window's jobs */
    atomic_int *failed;             /* ... and whether any of them failed */
};

static int read_chunk(const struct chunk_job *j)
{
    /* per-thread decode buffers, reused across chunks */
    static __thread unsigned char *raw = NULL, *scratch = NULL;
    static __thread size_t raw_cap = 0, scratch_cap = 0;
    struct gcn10_tiff *t = j->t;
    const size_t rawcap = (size_t)t->cw * t->ch * t->spp;
    struct chunk_clip c;

    if (rawcap > raw_cap) {
        unsigned char *g = realloc(raw, rawcap);

        if (!g)
            return -1;
        raw = g;
        raw_cap = rawcap;
    }
    if (!clip_chunk(t, j->cx, j->cy, &j->w, &c))
        return 0;
    {
        const uint32_t xs = c.xs, xe = c.xe, ys = c.ys, ye = c.ye, x_lo = c.x_lo, y_lo = c.y_lo;
        const uint32_t xoff = (uint32_t)j->w.xoff, yoff = (uint32_t)j->w.yoff;
        const size_t chunk_bytes = (size_t)t->cw * c.rows * t->spp;
        const unsigned char *from = raw;
        struct gcn10_cache_entry *held = NULL;

        /* an uncompressed chunk the window uses at most a quarter of (full-width strips): the wanted part of every
         * row straight from the file -- reading the chunk from its start to the last wanted pixel copied ~120 times
         * the bytes a block of a global raster needs */
        if (t->compression == 1 && t->predictor != 2 && t->spp == 1 &&
            (size_t)(xe - xs) * (ye - ys) * 4 <= chunk_bytes) {
            const uint64_t off = t->offsets[c.idx], cnt = t->counts[c.idx];

            if (cnt == 0) {
                for (uint32_t y = ys; y < ye; y++)
                    memset(j->dst + (size_t)(y - yoff) * j->dst_stride + (xs - xoff), 0, xe - xs);
                return 0;
            }
            if (!gcn10_tiff_chunk_in_file(t, c.idx) || cnt < ((size_t)(ye - 1 - y_lo) * t->cw + (xe - x_lo)))
                return -1;
            for (uint32_t y = ys; y < ye; y++)
                if (gcn10_pread_all(t->fd, j->dst + (size_t)(y - yoff) * j->dst_stride + (xs - xoff), xe - xs,
                                    off + (uint64_t)(y - y_lo) * t->cw + (xs - x_lo)) != 0)
                    return -1;
            return 0;
        }
        /* a compressed chunk the window uses at most a quarter of: through the cache, decoded in full */
        if (t->compression != 1 && (size_t)(xe - xs) * (ye - ys) * t->spp * 4 <= chunk_bytes &&
            gcn10_chunk_cache_enabled()) {
            held = gcn10_chunk_cache_get(t, c.idx, chunk_bytes);
            if (!held) {
                unsigned char *whole = malloc(chunk_bytes);

                if (whole && gcn10_tiff_decode_chunk(t, c.idx, whole, chunk_bytes, &scratch, &scratch_cap, c.rows,
                                                     chunk_bytes) == 0) {
                    held = gcn10_chunk_cache_put(t, c.idx, whole, chunk_bytes);
                    if (!held) {            /* not taken: copy from our own buffer below, then free it */
                        memcpy(raw, whole, chunk_bytes <= rawcap ? chunk_bytes : rawcap);
                        free(whole);
                    }
                }
                else {
                    free(whole);
                    return -1;
                }
            }
            if (held)
                from = held->data;
        }
        else if (gcn10_tiff_decode_chunk(t, c.idx, raw, rawcap, &scratch, &scratch_cap, c.rows,
                                         ((size_t)(ye - 1 - y_lo) * t->cw + (xe - x_lo)) * t->spp) != 0) {
            return -1;
        }
        for (uint32_t y = ys; y < ye; y++) {
            const unsigned char *s = from + ((size_t)(y - y_lo) * t->cw + (xs - x_lo)) * t->spp;
            uint8_t *d = j->dst + (size_t)(y - yoff) * j->dst_stride + (xs - xoff);

            if (t->spp == 1) {
                memcpy(d, s, xe - xs);
            }
            else {
                for (uint32_t x = 0; x < xe - xs; x++)
                    d[x] = s[(size_t)x * t->spp];
            }
        }
        if (held)
            gcn10_chunk_cache_release(held);
    }
    return 0;
}

static void chunk_job_run(void *arg)
{
    struct chunk_job *j = arg;

    if (read_chunk(j) != 0)
        atomic_store(j->failed, 1);
    gcn10_job_group_done(j->group);
    free(j);
}

int gcn10_tiff_read_window_mt(struct gcn10_tiff *t, int xoff, int yoff, int xcount, int ycount,
                              uint8_t *dst, size_t dst_stride, gcn10_pool *pool, char *err,
                              size_t errcap)
{
    const struct window w = { xoff, yoff, xcount, ycount };
    struct gcn10_job_group group;
    struct chunk_range r;
    atomic_int failed = 0;

    if (window_in_raster(t, &w, err, errcap) != 0)
        return -1;
    r = chunks_of_window(t, &w);
    gcn10_job_group_init(&group);
    for (uint32_t cy = r.cy0; cy <= r.cy1; cy++) {
        for (uint32_t cx = r.cx0; cx <= r.cx1; cx++) {
            struct chunk_job job = { t, cx, cy, w, dst, dst_stride, &group, &failed };
            struct chunk_job *j = pool ? malloc(sizeof *j) : NULL;

            if (!j) {               /* no pool (or no memory for the job): decode here */
                if (read_chunk(&job) != 0)
                    atomic_store(&failed, 1);
                continue;
            }
            *j = job;
            gcn10_job_group_add(&group, 1);
            gcn10_pool_submit(pool, chunk_job_run, j);
        }
    }
    gcn10_job_group_wait(&group);
    gcn10_job_group_destroy(&group);
    if (atomic_load(&failed)) {
        snprintf(err, errcap, "gdalrasterio error: cannot decode a %s of the window %d,%d %dx%d",
                 t->tiled ? "tile" : "strip", xoff, yoff, xcount, ycount);
        return -1;
    }
    return 0;
}

int gcn10_tiff_read_window(struct gcn10_tiff *t, int xoff, int yoff, int xcount, int ycount,
                           uint8_t *dst, size_t dst_stride, char *err, size_t errcap)
{
    return gcn10_tiff_read_window_mt(t, xoff, yoff, xcount, ycount, dst, dst_stride, NULL, err, errcap);
}

/* room for one more chunk in the plan: the slot, or NULL (out of memory) */
static struct gcn10_chunk_ref *plan_next_slot(struct gcn10_read_plan *plan)
{
    if (plan->n == plan->cap) {
        size_t cap = plan->cap ? plan->cap * 2 : 256;
        struct gcn10_chunk_ref *g = realloc(plan->chunks, cap * sizeof *g);

        if (!g)
            return NULL;
        plan->chunks = g;
        plan->cap = cap;
    }
    return &plan->chunks[plan->n];
}

/* The chunks of a window as they lie in the file, for the GPU side: DEFLATE chunks are inflated there, LZW chunks
 * decoded there when `codecs` has GCN10_CODEC_LZW, and TIFF predictor 2 (horizontal differencing) is undone there for
 * both; uncompressed chunks are only untiled there -- the Predictor tag does not apply to them (the host decoder
 * ignores it on them too).  Other codecs (PackBits; LZW without the bit) stay with the host reader (return 1).  Of
 * an uncompressed chunk only the bytes from the first wanted pixel to the last wanted pixel are staged. */
int gcn10_tiff_plan_window(struct gcn10_tiff *t, int xoff, int yoff, int xcount, int ycount, int dst_x,
                           int dst_y, unsigned codecs, struct gcn10_read_plan *plan, char *err, size_t errcap)
{
    const bool raw = t->compression == 1 && (codecs & GCN10_CODEC_RAW);
    const bool deflate = (t->compression == 8 || t->compression == 32946) && (codecs & GCN10_CODEC_DEFLATE);
    const bool lzw = t->compression == 5 && (codecs & GCN10_CODEC_LZW);
    const struct window w = { xoff, yoff, xcount, ycount };
    const char *const kind = t->tiled ? "tile" : "strip";
    struct chunk_range r;

    if ((!raw && !deflate && !lzw) || (t->predictor != 1 && t->predictor != 2) || t->spp != 1 ||
        t->bps != 8 || (uint64_t)t->cw * t->ch > ((uint64_t)1 << 28))
        return 1;
    if (window_in_raster(t, &w, err, errcap) != 0)
        return -1;
    r = chunks_of_window(t, &w);
    for (uint32_t cy = r.cy0; cy <= r.cy1; cy++) {
        for (uint32_t cx = r.cx0; cx <= r.cx1; cx++) {
            struct chunk_clip k;
            struct gcn10_chunk_ref *c;
            uint64_t off, cnt;

            if (!clip_chunk(t, cx, cy, &w, &k) || t->counts[k.idx] == 0)
                continue;               /* sparse chunk: reads as zeros */
            off = t->offsets[k.idx];
            cnt = t->counts[k.idx];
            if (!gcn10_tiff_chunk_in_file(t, k.idx)) {
                snprintf(err, errcap, "gdalrasterio error: a %s of the window %d,%d %dx%d lies outside the file",
                         kind, xoff, yoff, xcount, ycount);
                return -1;
            }
            if (cnt > 0x7fffffffu)
                return 1;
            c = plan_next_slot(plan);
            if (!c) {
                snprintf(err, errcap, "out of memory for the read plan");
                return -1;
            }
            c->fd = t->fd;
            c->file_off = off;
            c->nbytes = (uint32_t)cnt;
            c->chunk_w = t->cw;
            c->rows = k.rows;
            c->src_x = k.xs - k.x_lo;
            c->src_y = k.ys - k.y_lo;
            c->copy_w = k.xe - k.xs;
            c->copy_h = k.ye - k.ys;
            c->dst_x = (uint32_t)dst_x + (k.xs - (uint32_t)xoff);
            c->dst_y = (uint32_t)dst_y + (k.ys - (uint32_t)yoff);
            c->flags = raw ? GCN10_TILE_RAW
                           : (t->predictor == 2 ? GCN10_TILE_PREDICTOR2 : 0u) | (lzw ? GCN10_TILE_LZW : 0u);
            c->out_len = t->cw * k.rows;
            if (raw) {
                /* the bytes that matter: from the first wanted pixel to the last one */
                const uint64_t first = (uint64_t)c->src_y * t->cw + c->src_x;
                const uint64_t last = (uint64_t)(c->src_y + c->copy_h - 1u) * t->cw + c->src_x + c->copy_w;

                if (cnt < last) {       /* a chunk shorter than its pixels: what the host decoder refuses */
                    snprintf(err, errcap, "gdalrasterio error: cannot decode a %s of the window %d,%d %dx%d",
                             kind, xoff, yoff, xcount, ycount);
                    return -1;
                }
                /* full-width strips of a raster much wider than the window: most staged bytes would be
                 * other blocks' pixels -- the host reader copies rows instead */
                if (last - first > 4u * (uint64_t)c->copy_w * c->copy_h + ((uint64_t)1 << 20))
                    return 1;
                c->file_off = off + first;
                c->nbytes = (uint32_t)(last - first);
                c->out_len = c->nbytes;
                c->src_y = 0;
                c->src_x = 0;
            }
            else if (c->out_len > plan->max_chunk_bytes) {
                plan->max_chunk_bytes = c->out_len;
            }
            plan->n++;
            plan->staged_bytes += c->nbytes;
            plan->covered += (uint64_t)c->copy_w * c->copy_h;
        }
    }
    return 0;
}
