/* verify.c -- the verification mode of the run (config key verify=1, --verify; DESIGN.md "Verification").
 *
 * Nothing is written into the output directories.  For a block whose landcover and soil the input side has staged
 * exactly as for a write run, every selected raster file cn_rasters_<cond>/cn_<hc>_<arc>_<id>.tif is
 *   1. checked for its structure on the host (gcn10_verify_structure: the file, the TIFF, one band of Byte, the
 *      window's size and geotransform, every chunk inside the file, the overview directories' sizes),
 *   2. read strip by strip AS IT LIES IN THE FILE: the chunks that cover the strip are planned (gcn10_tiff_plan_window
 *      with DEFLATE | RAW | LZW), read into pinned memory by the I/O pool, copied to the device and decoded there by
 *      gcn10_gpu_inflate_tiles -- the chunks of all 18 files in one call -- into 18 strip buffers,
 *   3. compared there with what the program computes now: gcn10_gpu_verify_strip over the strip's landcover and the
 *      prepared soil (the expected rasters are never made); overview levels the same way, a nearest level as a block
 *      of its own, an average level against gcn10_gpu_overview_average's buffers (gcn10_gpu_verify_buffers).
 * A window the planner leaves to the host reader (PackBits, very wide raw strips) is decoded by it and uploaded.
 * The per-chunk status words of the decoder are findings: a stream that does not decode makes its file unreadable,
 * it never faults the device.  At the bottom: the run's closing summary and verify_failed_blocks.txt.
 */
#include "pipeline_internal.h"

#include <errno.h>
#include <limits.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#define wlog gcn10_wlog

enum { V_LEVELS = GCN10_COG_MAX_LEVELS + 1, V_STAGE = 2 };
/* device memory of the 18 decode buffers of a strip: bounds the strip height together with strip_rows */
#define V_GOT_BYTES ((size_t)1 << 30)

static const char *const finding_names[] = { "ok", "missing", "not a TIFF", "not 1 band Byte", "size", "geotransform",
                                             "chunk", "overview size", "decode", "pixels" };

/* ------------------------------------------------------------------------ */
/* structure of one file                                                     */
/* ------------------------------------------------------------------------ */

/* The checks of gcn10_verify_structure; the readers of the raster and of its overview directories stay open in
 * lv[0 .. *n_levels] when the finding is GCN10_VERIFY_OK (closed otherwise). */
static int open_checked(const char *path, int W, int H, const double gt[6], struct gcn10_tiff *lv[V_LEVELS],
                        int *n_levels, int *n_beyond, char *reason, size_t cap)
{
    char err[1024] = "";
    int why = 0, finding = GCN10_VERIFY_OK, fw, fh, n = 0;
    double fgt[6];
    uint64_t idx, off, cnt;

    memset(lv, 0, V_LEVELS * sizeof lv[0]);
    *n_levels = 0;
    *n_beyond = 0;
    lv[0] = gcn10_tiff_open_reader_ifd(path, 0, &why, err, sizeof err);
    if (!lv[0]) {
        if (why == GCN10_TIFF_E_MISSING) {
            snprintf(reason, cap, "no such file");
            return GCN10_VERIFY_MISSING;
        }
        snprintf(reason, cap, "%s", err);
        return why == GCN10_TIFF_E_NOT_BYTE ? GCN10_VERIFY_NOT_BYTE : GCN10_VERIFY_NOT_TIFF;
    }
    gcn10_tiff_reader_info(lv[0], &fw, &fh, fgt);
    if (gcn10_tiff_reader_samples(lv[0]) != 1) {
        snprintf(reason, cap, "%d samples per pixel, not 1 band of Byte", gcn10_tiff_reader_samples(lv[0]));
        finding = GCN10_VERIFY_NOT_BYTE;
    }
    else if (fw != W || fh != H) {
        snprintf(reason, cap, "size %dx%d, the block's window is %dx%d", fw, fh, W, H);
        finding = GCN10_VERIFY_SIZE;
    }
    else if (memcmp(fgt, gt, sizeof fgt) != 0) {
        /* the six doubles the writer stores come back from the reader bit for bit (origin = tiepoint, pixel
         * size = scale), so anything but equality is another georeference */
        snprintf(reason, cap, "geotransform {%.17g, %.17g, %.17g, %.17g, %.17g, %.17g}, the window's is "
                 "{%.17g, %.17g, %.17g, %.17g, %.17g, %.17g}", fgt[0], fgt[1], fgt[2], fgt[3], fgt[4], fgt[5],
                 gt[0], gt[1], gt[2], gt[3], gt[4], gt[5]);
        finding = GCN10_VERIFY_GEOTRANSFORM;
    }
    else if (gcn10_tiff_check_chunks(lv[0], &idx, &off, &cnt) != 0) {
        snprintf(reason, cap, "chunk %llu: offset %llu + %llu bytes %s", (unsigned long long)idx,
                 (unsigned long long)off, (unsigned long long)cnt,
                 cnt == 0 ? "(no bytes where pixels are expected)" : "lies beyond the end of the file");
        finding = GCN10_VERIFY_CHUNK;
    }
    /* the overview directories behind it: each must be the halving rule's size and lie inside the file */
    while (finding == GCN10_VERIFY_OK && gcn10_tiff_reader_has_next(lv[n])) {
        struct gcn10_tiff *t;

        if (n + 1 >= V_LEVELS) {
            (*n_beyond)++;              /* more levels than the program makes: counted as not checked */
            break;
        }
        t = gcn10_tiff_open_reader_ifd(path, n + 1, &why, err, sizeof err);
        if (!t) {
            snprintf(reason, cap, "overview %d: %s", n + 1, err);
            finding = why == GCN10_TIFF_E_NOT_BYTE ? GCN10_VERIFY_NOT_BYTE : GCN10_VERIFY_NOT_TIFF;
            break;
        }
        lv[++n] = t;
        gcn10_tiff_reader_info(t, &fw, &fh, fgt);
        if (gcn10_tiff_reader_samples(t) != 1) {
            snprintf(reason, cap, "overview %d: %d samples per pixel, not 1 band of Byte", n, gcn10_tiff_reader_samples(t));
            finding = GCN10_VERIFY_NOT_BYTE;
        }
        else if (fw != gcn10_level_dim(W, n) || fh != gcn10_level_dim(H, n)) {
            snprintf(reason, cap, "overview %d: size %dx%d, level %d of %dx%d is %dx%d", n, fw, fh, n, W, H,
                     gcn10_level_dim(W, n), gcn10_level_dim(H, n));
            finding = GCN10_VERIFY_OVERVIEW;
        }
        else if (gcn10_tiff_check_chunks(t, &idx, &off, &cnt) != 0) {
            snprintf(reason, cap, "overview %d, chunk %llu: offset %llu + %llu bytes %s", n, (unsigned long long)idx,
                     (unsigned long long)off, (unsigned long long)cnt,
                     cnt == 0 ? "(no bytes where pixels are expected)" : "lies beyond the end of the file");
            finding = GCN10_VERIFY_CHUNK;
        }
    }
    if (finding != GCN10_VERIFY_OK) {
        for (int k = 0; k < V_LEVELS; k++) {
            gcn10_tiff_close_reader(lv[k]);
            lv[k] = NULL;
        }
        return finding;
    }
    *n_levels = n;
    return GCN10_VERIFY_OK;
}

int gcn10_verify_structure(const char *path, int xsize, int ysize, const double gt[6], int *n_levels, char *reason,
                           size_t reason_cap)
{
    struct gcn10_tiff *lv[V_LEVELS];
    char text[1024] = "";
    int n = 0, beyond = 0;
    const int finding = open_checked(path, xsize, ysize, gt, lv, &n, &beyond, text, sizeof text);

    for (int k = 0; k < V_LEVELS; k++)
        gcn10_tiff_close_reader(lv[k]);
    if (n_levels)
        *n_levels = n + beyond;
    if (reason && reason_cap)
        snprintf(reason, reason_cap, "%s", text);
    return finding;
}

/* ------------------------------------------------------------------------ */
/* the worker's verify state                                                 */
/* ------------------------------------------------------------------------ */

struct vfile {
    int k;                                  /* raster index cond*9 + hc*3 + arc */
    struct gcn10_tiff *lv[V_LEVELS];
    int n_levels;
    int finding;                            /* GCN10_VERIFY_* */
    char reason[1200];
};

struct gcn10_verify_state {
    uint8_t *d_got;                         /* n_sel strip buffers */
    size_t got_cap;
    uint8_t *d_comp;
    size_t comp_cap;
    struct gcn10_stager stage;              /* V_STAGE pinned buffers of RING_BYTES, copies on s_kernel */
    struct gcn10_job_list jl;               /* the strip's chunks of all files: the decoder's jobs, */
    struct gcn10_chunk_ref *chunks;         /* ... where they lie and whose they are */
    int *owner;
    gcn10_verify_count *d_counts, *h_counts;    /* [V_LEVELS][GCN10_N_RASTERS]; h_counts pinned */
    uint8_t *h_rows;                        /* a host-decoded strip on its way up */
    size_t h_rows_cap;
};

static int state_setup(struct worker *w)
{
    const struct gcn10_gpu_api *g = w->run->gpu;
    struct gcn10_verify_state *v;
    const size_t n_counts = (size_t)V_LEVELS * GCN10_N_RASTERS;

    if (w->verify)
        return 0;
    v = calloc(1, sizeof *v);
    if (!v) {
        wlog(w, "ERROR", true, "malloc failed for the verifier");
        return -1;
    }
    w->verify = v;
    GPU_OR_RETURN(w, -1, gcn10_stager_setup(&v->stage, g, w->ctx, w->run->pool, &w->run->pinned_bytes, V_STAGE,
                                            RING_BYTES));
    GPU_OR_RETURN(w, -1, g->malloc(w->ctx, n_counts * sizeof *v->d_counts, (void **)&v->d_counts));
    GPU_OR_RETURN(w, -1, g->host_alloc(w->ctx, n_counts * sizeof *v->h_counts, (void **)&v->h_counts));
    return 0;
}

static void verify_teardown(struct worker *w)
{
    const struct gcn10_gpu_api *g = w->run->gpu;
    struct gcn10_verify_state *v = w->verify;

    if (!v)
        return;
    if (v->d_got) g->free(w->ctx, v->d_got);
    if (v->d_comp) g->free(w->ctx, v->d_comp);
    gcn10_stager_teardown(&v->stage);
    gcn10_job_list_free(g, w->ctx, &v->jl);
    if (v->d_counts) g->free(w->ctx, v->d_counts);
    if (v->h_counts) g->host_free(w->ctx, v->h_counts);
    free(v->chunks);
    free(v->owner);
    free(v->h_rows);
    free(v);
    w->verify = NULL;
}

/* room for n chunks in the strip's lists; the first `keep` entries (the files planned so far) stay */
static int jobs_ensure(struct worker *w, size_t n, size_t keep)
{
    const struct gcn10_gpu_api *g = w->run->gpu;
    struct gcn10_verify_state *v = w->verify;
    struct gcn10_chunk_ref *c;
    int *o;

    if (n <= v->jl.cap)
        return 0;
    n = n * 2 > 4096 ? n * 2 : 4096;
    /* the caller appends while it plans: the host lists are kept, the device-side arrays are rewritten per strip */
    c = realloc(v->chunks, n * sizeof *c);
    if (c)
        v->chunks = c;
    o = realloc(v->owner, n * sizeof *o);
    if (o)
        v->owner = o;
    if (!c || !o) {
        wlog(w, "ERROR", true, "malloc failed for the verifier's read plan");
        return -1;
    }
    GPU_OR_RETURN(w, -1, g->stream_sync(w->ctx, w->s_kernel));
    GPU_OR_RETURN(w, -1, gcn10_job_list_ensure(g, w->ctx, &v->jl, n, keep));
    return 0;
}

/* ------------------------------------------------------------------------ */
/* one level of a block                                                      */
/* ------------------------------------------------------------------------ */

static void set_finding(struct vfile *f, int finding, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
static void set_finding(struct vfile *f, int finding, const char *fmt, ...)
{
    va_list ap;

    if (f->finding != GCN10_VERIFY_OK)
        return;                             /* the first finding of a file is the one reported */
    f->finding = finding;
    va_start(ap, fmt);
    vsnprintf(f->reason, sizeof f->reason, fmt, ap);
    va_end(ap);
}

/* Rows per strip of a level Wk pixels wide: what strip_rows says, as far as the n_sel decode buffers fit
 * V_GOT_BYTES; whole tile rows, at least one. */
static int rows_per_strip(const struct run *r, size_t stride)
{
    size_t rows = V_GOT_BYTES / ((size_t)r->n_sel * stride);

    rows = rows / TILE * TILE;
    if (rows > (size_t)r->strip_rows)
        rows = (size_t)r->strip_rows;
    return rows < TILE ? TILE : (int)rows;
}

/* Level `level` (Wk x Hk) of the block's files against d_esa / d_cj (the level's landcover and soil rows, the tile of
 * width Wk prepared) or, with `want` (per selected raster q: the level's expected raster, rows Wk apart), against
 * those buffers.  Files with a finding are left out.  0, or -1 for a device error (logged). */
static int verify_level(struct worker *w, struct vfile *files, int level, int Wk, int Hk, const uint8_t *d_esa,
                        const int32_t *d_cj, uint8_t *const *want)
{
    struct run *r = w->run;
    const struct gcn10_gpu_api *g = r->gpu;
    struct gcn10_verify_state *v = w->verify;
    const size_t stride = ((size_t)Wk + 15) & ~(size_t)15;
    const int strip = rows_per_strip(r, stride);
    const size_t slot = stride * (size_t)(strip < Hk ? strip : Hk);
    gcn10_verify_count *counts = v->d_counts + (size_t)level * GCN10_N_RASTERS;
    const unsigned codecs = r->inflate_codecs | GCN10_CODEC_DEFLATE | GCN10_CODEC_RAW;
    int rc = -1;

    if (gcn10_ensure_dev_on(w, w->ctx, (void **)&v->d_got, &v->got_cap, slot * (size_t)r->n_sel + 16) != 0)
        return -1;
    for (int y0 = 0; y0 < Hk; y0 += strip) {
        const int rows = Hk - y0 < strip ? Hk - y0 : strip;
        const uint8_t *got[GCN10_N_RASTERS] = { 0 }, *exp[GCN10_N_RASTERS] = { 0 };
        unsigned mask = 0;
        size_t n = 0, comp_bytes = 0;
        uint32_t chunk_bytes = 16;
        bool sparse = false;

        /* plan: the chunks of every file that cover the strip */
        for (int q = 0; q < r->n_sel; q++) {
            struct vfile *f = &files[q];
            struct gcn10_read_plan plan;
            char err[1024] = "";
            int prc;

            got[f->k] = v->d_got + (size_t)q * slot;
            if (want)
                exp[f->k] = want[q] + (size_t)y0 * (size_t)Wk;
            if (f->finding != GCN10_VERIFY_OK || level > f->n_levels)
                continue;
            memset(&plan, 0, sizeof plan);
            prc = gcn10_tiff_plan_window(f->lv[level], 0, y0, Wk, rows, 0, 0, codecs, &plan, err, sizeof err);
            if (prc < 0) {
                set_finding(f, GCN10_VERIFY_CHUNK, "level %d, rows %d..%d: %s", level, y0, y0 + rows - 1, err);
                gcn10_read_plan_free(&plan);
                continue;
            }
            if (prc > 0) {
                /* the host reader's codecs and shapes: decoded here, uploaded; slower, the same answer */
                gcn10_read_plan_free(&plan);
                if (v->h_rows_cap < stride * (size_t)rows) {
                    free(v->h_rows);
                    v->h_rows = malloc(stride * (size_t)rows);
                    v->h_rows_cap = v->h_rows ? stride * (size_t)rows : 0;
                }
                if (!v->h_rows) {
                    wlog(w, "ERROR", true, "malloc failed for a host-decoded strip");
                    goto out;
                }
                if (gcn10_tiff_read_window(f->lv[level], 0, y0, Wk, rows, v->h_rows, stride, err, sizeof err) != 0) {
                    set_finding(f, GCN10_VERIFY_DECODE, "level %d, rows %d..%d: %s", level, y0, y0 + rows - 1, err);
                    continue;
                }
                /* pageable memory: the copy is done with the buffer when the call returns */
                if (g->memcpy_h2d(w->ctx, v->d_got + (size_t)q * slot, v->h_rows, stride * (size_t)rows, w->s_kernel) != 0 ||
                    g->stream_sync(w->ctx, w->s_kernel) != 0)
                    goto gpu_fail;
                mask |= 1u << f->k;
                continue;
            }
            if (jobs_ensure(w, n + plan.n, n) != 0) {
                gcn10_read_plan_free(&plan);
                goto out;
            }
            for (size_t i = 0; i < plan.n; i++) {
                const struct gcn10_chunk_ref *c = &plan.chunks[i];

                v->chunks[n] = *c;
                v->owner[n] = q;
                gcn10_inflate_job_from_chunk(&v->jl.h_jobs[n], c, comp_bytes,
                                             (uint64_t)q * slot + (uint64_t)c->dst_y * stride + c->dst_x);
                v->jl.h_status[n] = 0xffffffffu;
                comp_bytes += gcn10_chunk_slot(c->nbytes);
                n++;
            }
            if (plan.max_chunk_bytes > chunk_bytes)
                chunk_bytes = plan.max_chunk_bytes;
            if (plan.covered < (uint64_t)Wk * (uint64_t)rows)
                sparse = true;
            /* (the readers of this block stay open until it is done: the chunks' descriptors stay valid) */
            gcn10_read_plan_free(&plan);
            mask |= 1u << f->k;
        }
        if (mask == 0)
            continue;
        if (n > 0) {
            if (gcn10_ensure_dev_on(w, w->ctx, (void **)&v->d_comp, &v->comp_cap, comp_bytes + 16) != 0)
                goto out;
            if (sparse && g->memset(w->ctx, v->d_got, 0, slot * (size_t)r->n_sel, w->s_kernel) != 0)
                goto gpu_fail;
            if (gcn10_stager_stage(&v->stage, v->chunks, v->jl.h_jobs, n, v->d_comp, w->s_kernel, v->jl.bad) != 0)
                goto gpu_fail;
            for (size_t i = 0; i < n; i++)
                if (v->jl.bad[i]) {
                    /* a chunk that cannot be read is not handed to the decoder: an empty window */
                    v->jl.h_jobs[i].copy_w = v->jl.h_jobs[i].copy_h = 0;
                    v->jl.h_jobs[i].in_len = 0;
                    v->jl.h_jobs[i].flags = GCN10_TILE_RAW;
                    v->jl.h_jobs[i].out_len = 0;
                }
            if (g->memcpy_h2d(w->ctx, v->jl.d_jobs, v->jl.h_jobs, n * sizeof *v->jl.h_jobs, w->s_kernel) != 0 ||
                g->memcpy_h2d(w->ctx, v->jl.d_status, v->jl.h_status, n * 4, w->s_kernel) != 0 ||
                g->inflate_tiles(w->ctx, v->d_comp, v->jl.d_jobs, (int)n, chunk_bytes, v->d_got, stride, v->jl.d_status,
                                 w->s_kernel) != 0 ||
                g->memcpy_d2h(w->ctx, v->jl.h_status, v->jl.d_status, n * 4, w->s_kernel) != 0)
                goto gpu_fail;
        }
        if (want) {
            if (g->verify_buffers(w->ctx, exp, (size_t)Wk, got, stride, Wk, rows, y0, mask, counts, w->s_kernel) != 0)
                goto gpu_fail;
        }
        else if (g->verify_strip(w->ctx, d_esa + (size_t)y0 * (size_t)Wk, Wk, rows, d_cj + y0, r->cond_mask,
                                 r->table_mask, got, stride, y0, counts, w->s_kernel) != 0) {
            goto gpu_fail;
        }
        /* the strip's buffers, job lists and staging are reused by the next one */
        if (g->stream_sync(w->ctx, w->s_kernel) != 0)
            goto gpu_fail;
        gcn10_stager_idle(&v->stage);
        for (size_t i = 0; i < n; i++) {
            struct vfile *f = &files[v->owner[i]];
            const struct gcn10_chunk_ref *c = &v->chunks[i];

            if (v->jl.bad[i])
                set_finding(f, GCN10_VERIFY_CHUNK, "level %d: the %u bytes of the chunk at x=%u y=%d cannot be read%s",
                            level, c->nbytes, c->dst_x, y0 + (int)c->dst_y, v->jl.bad[i] == 2 ? " (too large to stage)" : "");
            else if (v->jl.h_status[i] != 0)
                set_finding(f, GCN10_VERIFY_DECODE, "level %d: the chunk at x=%u y=%d (%u bytes at offset %llu) does "
                            "not decode, status %u", level, c->dst_x, y0 + (int)c->dst_y, c->nbytes,
                            (unsigned long long)c->file_off, v->jl.h_status[i]);
        }
    }
    rc = 0;
    goto out;

gpu_fail:
    wlog(w, "ERROR", true, "gpu: %s", g->last_error());
out:
    return rc;
}

/* ------------------------------------------------------------------------ */
/* one block                                                                 */
/* ------------------------------------------------------------------------ */

/* the overview levels of the files against nearest-neighbour levels: each a block of its own, made as the writer
 * makes it (levels.c) */
static int verify_nearest_levels(struct worker *w, struct block_in *in, struct vfile *files, int L)
{
    for (int k = L; k >= 1; k--) {
        const int32_t *d_cj;
        int Wk, Hk;

        if (gcn10_level_nearest(w, in, k, &Wk, &Hk, &d_cj) != 0 ||
            verify_level(w, files, k, Wk, Hk, w->d_ov, d_cj, NULL) != 0)     /* (ends with its kernels done) */
            return -1;
    }
    return 0;
}

/* ... against averaged levels: the pyramid of every selected raster as the writer makes it (the block's tile is
 * prepared), then level by level against those buffers */
static int verify_average_levels(struct worker *w, struct block_in *in, struct vfile *files, int L)
{
    struct run *r = w->run;
    uint8_t *levels[GCN10_N_RASTERS * GCN10_COG_MAX_LEVELS];

    if (gcn10_levels_average(w, in, L, r->strip_rows, levels) != 0)
        return -1;
    for (int k = L; k >= 1; k--) {
        uint8_t *want[GCN10_N_RASTERS];

        for (int q = 0; q < r->n_sel; q++)
            want[q] = levels[q * L + k - 1];
        if (verify_level(w, files, k, gcn10_level_dim(in->W, k), gcn10_level_dim(in->H, k), NULL, NULL, want) != 0)
            return -1;
    }
    return 0;
}

static void raster_name(char *out, size_t cap, int k)
{
    snprintf(out, cap, "%s/%s/%s", gcn10_conds[k / 9], gcn10_hcs[(k % 9) / 3], gcn10_arcs[k % 3]);
}

static void block_failed(struct run *r, int block_id)
{
    pthread_mutex_lock(&r->verify_mu);
    if (r->verify_n_failed < r->verify_failed_cap)
        r->verify_failed[r->verify_n_failed++] = block_id;
    pthread_mutex_unlock(&r->verify_mu);
}

static void verify_block_unreadable(struct worker *w, int block_id)
{
    struct run *r = w->run;

    wlog(w, "ERROR", true, "UNREADABLE block %d: its landcover or soil window could not be read, %d rasters not verified",
         block_id, r->n_sel);
    atomic_fetch_add(&r->verify_n_bad, r->n_sel);
    block_failed(r, block_id);
}

static int verify_block(struct worker *w, struct block_in *in)
{
    struct run *r = w->run;
    const struct gcn10_gpu_api *g = r->gpu;
    const int W = in->W, H = in->H, block_id = in->block_id;
    struct vfile files[GCN10_N_RASTERS];
    struct gcn10_verify_state *v;
    int L = 0, rc = -1, n_beyond_total = 0;
    bool any_failed = false;

    memset(files, 0, sizeof files);
    if (state_setup(w) != 0)
        return -1;
    v = w->verify;

    /* 1. the files' structure, on the host, before any pixel work */
    for (int q = 0; q < r->n_sel; q++) {
        struct vfile *f = &files[q];
        char path[PATH_MAX];
        int beyond = 0;

        f->k = r->sel[q];
        snprintf(path, sizeof path, "cn_rasters_%s/cn_%s_%s_%d.tif", gcn10_conds[f->k / 9], gcn10_hcs[(f->k % 9) / 3],
                 gcn10_arcs[f->k % 3], block_id);                           /* src/cn.c:308 */
        f->finding = open_checked(path, W, H, in->gt, f->lv, &f->n_levels, &beyond, f->reason, sizeof f->reason);
        n_beyond_total += beyond;
        if (beyond) {
            char name[64];

            raster_name(name, sizeof name, f->k);
            wlog(w, "ERROR", true, "block %d: %s: overview levels beyond %d not checked", block_id, name,
                 GCN10_COG_MAX_LEVELS);
        }
        if (f->finding == GCN10_VERIFY_OK && f->n_levels > L)
            L = f->n_levels;
    }

    /* 2. the block on the device, as for a write run */
    switch (gcn10_block_take(w, in)) {
    case GCN10_BLOCK_DEVICE_ERROR:
        goto gpu_fail;
    case GCN10_BLOCK_UNREADABLE:
        verify_block_unreadable(w, block_id);
        rc = 0;
        goto out;
    }
    for (size_t i = 0; i < (size_t)V_LEVELS * GCN10_N_RASTERS; i++)
        v->h_counts[i] = (gcn10_verify_count){ 0, UINT64_MAX, 0, 0 };
    if (g->memcpy_h2d(w->ctx, v->d_counts, v->h_counts, (size_t)V_LEVELS * GCN10_N_RASTERS * sizeof *v->h_counts,
                      w->s_kernel) != 0)
        goto gpu_fail;

    /* 3. overview levels (nearest ones prepare their own tiles, so they come first), then the raster itself */
    if (L > 0 && !r->ov_average) {
        if (verify_nearest_levels(w, in, files, L) != 0)
            goto out;
    }
    if (g->prepare_tile(w->ctx, in->d_coarse, in->hsx, in->hsy, in->d_ci, W, w->s_kernel) != 0)
        goto gpu_fail;
    if (L > 0 && r->ov_average) {
        if (verify_average_levels(w, in, files, L) != 0)
            goto out;
    }
    if (verify_level(w, files, 0, W, H, in->d_block, in->d_cj, NULL) != 0)
        goto out;
    if (g->memcpy_d2h(w->ctx, v->h_counts, v->d_counts, (size_t)V_LEVELS * GCN10_N_RASTERS * sizeof *v->h_counts,
                      w->s_kernel) != 0 ||
        g->stream_sync(w->ctx, w->s_kernel) != 0)
        goto gpu_fail;

    /* 4. one line per file */
    for (int q = 0; q < r->n_sel; q++) {
        struct vfile *f = &files[q];
        char name[64];
        uint64_t n_diff = 0;
        int first_level = -1;

        raster_name(name, sizeof name, f->k);
        if (f->finding == GCN10_VERIFY_MISSING) {
            wlog(w, "ERROR", true, "MISSING block %d: %s", block_id, name);
            atomic_fetch_add(&r->verify_n_missing, 1);
            any_failed = true;
            continue;
        }
        if (f->finding != GCN10_VERIFY_OK) {
            wlog(w, "ERROR", true, "UNREADABLE block %d: %s: %s: %s", block_id, name, finding_names[f->finding], f->reason);
            atomic_fetch_add(&r->verify_n_bad, 1);
            any_failed = true;
            continue;
        }
        for (int k = 0; k <= f->n_levels; k++) {
            const gcn10_verify_count *c = &v->h_counts[(size_t)k * GCN10_N_RASTERS + f->k];

            n_diff += c->mismatches;
            if (c->mismatches && first_level < 0)
                first_level = k;
        }
        if (n_diff) {
            const gcn10_verify_count *c = &v->h_counts[(size_t)first_level * GCN10_N_RASTERS + f->k];

            wlog(w, "ERROR", true, "MISMATCH block %d: %s: %llu pixels differ, first at x=%u y=%u (level %d): file %u, "
                 "expected %u", block_id, name, (unsigned long long)n_diff, (unsigned)(c->first & 0xffffffffu),
                 (unsigned)(c->first >> 32), first_level, c->got, c->want);
            atomic_fetch_add(&r->verify_n_bad, 1);
            any_failed = true;
            continue;
        }
        wlog(w, "INFO", false, "verified block %d: %s", block_id, name);
        atomic_fetch_add(&r->verify_n_ok, 1);
    }
    atomic_fetch_add(&r->verify_n_unchecked, n_beyond_total);
    if (any_failed)
        block_failed(r, block_id);
    rc = 0;
    goto out;

gpu_fail:
    wlog(w, "ERROR", true, "gpu: %s", g->last_error());
out:
    if (w->ctx)
        g->stream_sync(w->ctx, w->s_kernel);
    gcn10_stager_idle(&v->stage);
    for (int q = 0; q < r->n_sel; q++)
        for (int k = 0; k < V_LEVELS; k++)
            gcn10_tiff_close_reader(files[q].lv[k]);
    return rc;
}

static int by_int(const void *a, const void *b)
{
    const int x = *(const int *)a, y = *(const int *)b;

    return x < y ? -1 : (x > y ? 1 : 0);
}

/* The end of a verify run: the closing console line and <log_dir>/verify_failed_blocks.txt, the ids of the blocks
 * with a bad or missing file, ascending, one per line (what -l reads).  Under an MPI launcher every process leaves
 * its counts and ids in "<log_dir>/.verify_<job>_<rank>" BEFORE the closing barrier, and launcher rank 0 merges
 * them behind it, the way it prints the run's totals.  Returns the exit code: 2 when it knows of a bad or missing file. */
static void verify_leave_part(struct run *r)
{
    char job[96], path[PATH_MAX];
    FILE *f;

    gcn10_job_tag(job);
    snprintf(path, sizeof path, "%s/.verify_%s_%d", r->cfg.log_dir, job, r->outer_rank);
    f = fopen(path, "w");
    if (!f)
        return;
    fprintf(f, "%d %d %d %d %d %d\n", r->n_blocks, atomic_load(&r->verify_n_ok), atomic_load(&r->verify_n_bad),
            atomic_load(&r->verify_n_missing), atomic_load(&r->verify_n_unchecked), r->verify_n_failed);
    for (int i = 0; i < r->verify_n_failed; i++)
        fprintf(f, "%d\n", r->verify_failed[i]);
    fclose(f);
}

static int verify_summary(struct run *r, gcn10_log *log0)
{
    int blocks = r->n_blocks, ok = atomic_load(&r->verify_n_ok), bad = atomic_load(&r->verify_n_bad);
    int missing = atomic_load(&r->verify_n_missing), unchecked = atomic_load(&r->verify_n_unchecked);
    int *ids = r->verify_failed, n_ids = r->verify_n_failed;
    char path[PATH_MAX], msg[PATH_MAX + 64];
    FILE *f;

    if (r->outer_size > 1) {
        char job[96];

        if (r->outer_rank != 0)
            return bad + missing > 0 ? 2 : 0;
        gcn10_job_tag(job);
        for (int p = 1; p < r->outer_size; p++) {
            int b, o, x, m, u, n;

            snprintf(path, sizeof path, "%s/.verify_%s_%d", r->cfg.log_dir, job, p);
            f = fopen(path, "r");
            if (!f)
                continue;               /* (the barrier has said so: "some processes did not report in time") */
            if (fscanf(f, "%d %d %d %d %d %d", &b, &o, &x, &m, &u, &n) == 6 && n >= 0) {
                int *g = realloc(ids == r->verify_failed ? NULL : ids, (size_t)(n_ids + n + 1) * sizeof *g);

                if (g) {
                    if (ids == r->verify_failed && n_ids > 0)
                        memcpy(g, r->verify_failed, (size_t)n_ids * sizeof *g);
                    ids = g;
                    for (int i = 0; i < n && fscanf(f, "%d", &ids[n_ids]) == 1; i++)
                        n_ids++;
                }
                blocks += b;
                ok += o;
                bad += x;
                missing += m;
                unchecked += u;
            }
            fclose(f);
            unlink(path);
        }
        snprintf(path, sizeof path, "%s/.verify_%s_0", r->cfg.log_dir, job);
        unlink(path);
    }
    if (n_ids > 0)
        qsort(ids, (size_t)n_ids, sizeof *ids, by_int);
    snprintf(path, sizeof path, "%s/verify_failed_blocks.txt", r->cfg.log_dir);
    f = fopen(path, "w");
    if (f) {
        for (int i = 0; i < n_ids; i++)
            if (i == 0 || ids[i] != ids[i - 1])
                fprintf(f, "%d\n", ids[i]);
        fclose(f);
    }
    else {
        snprintf(msg, sizeof msg, "cannot write %s", path);
        gcn10_log_message(log0, "ERROR", msg, true);
    }
    snprintf(msg, sizeof msg, "verify: %d blocks, %d files verified, %d bad, %d missing, %d overview levels not checked",
             blocks, ok, bad, missing, unchecked);
    gcn10_log_message(log0, bad + missing ? "ERROR" : "INFO", msg, true);
    if (ids != r->verify_failed)
        free(ids);
    return bad + missing > 0 ? 2 : 0;
}

const struct gcn10_mode gcn10_mode_verify = {
    .block = verify_block, .block_unreadable = verify_block_unreadable, .worker_teardown = verify_teardown,
    .leave_part = verify_leave_part, .finish = verify_summary,
};
