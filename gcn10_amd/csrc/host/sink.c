/* sink.c -- the sink of the per-block pipeline: what happens to a strip once the encoder is done with it.
 *
 * The worker hands a finished strip over (gcn10_sink_drain); pool jobs append it to the rasters' files -- already
 * compressed tiles as one extent per raster behind a gate job that waits for the copy-back (GPU encoders), or tile
 * rows deflated here (host zlib) -- and close the files at the end of the block (gcn10_sink_finish_files).  A strip
 * buffer counts its jobs (strip_buf.jobs); gcn10_sink_wait is the wait for them.  The strip buffers themselves and
 * the grow-only device / pinned buffers of a worker live here too.
 */
#include "pipeline_internal.h"

#include <stdlib.h>
#include <string.h>

#define now_seconds gcn10_now_seconds
#define wlog gcn10_wlog

/* ---- the four kinds of job ---- */

struct tile_job {
    struct worker *w;
    struct strip_buf *b;
    gcn10_tiff_writer *tif;
    const uint8_t *strip;                   /* pinned strip of one raster */
    int W, H;                               /* raster size */
    int y0;                                 /* first raster row of the strip */
    int ty;                                 /* tile row (global) */
};

static void tile_row_job(void *arg)
{
    struct tile_job *j = arg;
    struct run *r = j->w->run;
    uint8_t z[TILE * TILE + TILE * TILE / 1000 + 64];       /* >= compressBound(65536) */
    int across = gcn10_tiff_tiles_across(j->tif);
    int row0 = j->ty * TILE;
    int vh = j->H - row0 < TILE ? j->H - row0 : TILE;

    for (int tx = 0; tx < across; tx++) {
        int vw = j->W - tx * TILE < TILE ? j->W - tx * TILE : TILE;
        const uint8_t *src = j->strip + (size_t)(row0 - j->y0) * (size_t)j->W + (size_t)tx * TILE;
        size_t n = gcn10_deflate_tile(src, (size_t)j->W, vw, vh, r->deflate_level, z, sizeof z);

        if (n == 0 || gcn10_tiff_put_tile(j->tif, tx, j->ty, z, n) != 0) {
            atomic_store(&j->w->failed, true);
            break;
        }
    }
    gcn10_job_group_done(&j->b->jobs);
    free(j);
}

/* GPU-deflate sink: append the already compressed tiles of one raster */
struct put_job {
    struct worker *w;
    struct strip_buf *b;
    gcn10_tiff_writer *tif;
    int raster, ty0, across, down;          /* tile rows ty0 .. ty0+down of the raster */
};

static void put_tiles_job(void *arg)
{
    struct put_job *j = arg;
    const uint32_t *tab = j->b->h_table + (size_t)j->raster * (size_t)j->across * (size_t)j->down * 2;
    const size_t n = (size_t)j->across * (size_t)j->down;
    int *txs = malloc(n * sizeof *txs), *tys = malloc(n * sizeof *tys);
    const void **data = malloc(n * sizeof *data);
    uint32_t *sizes = malloc(n * sizeof *sizes), *rel = malloc(n * sizeof *rel);
    bool ok = txs && tys && data && sizes && rel;
    bool extent = true;             /* the streams lie back to back in tile order (16-byte slots) */
    uint32_t first = 0, end = 0;

    for (int ty = 0; ok && ty < j->down; ty++) {
        for (int tx = 0; tx < j->across; tx++) {
            const size_t i = (size_t)ty * j->across + tx;
            const uint32_t off = tab[i * 2], size = tab[i * 2 + 1];

            /* the host copy holds exactly the `used` bytes the encoder produced, not arena_cap */
            if (off == 0xffffffffu || size == 0 || (size_t)off + size > j->b->h_tiles_used) {
                ok = false;
                break;
            }
            txs[i] = tx;
            tys[i] = j->ty0 + ty;
            data[i] = j->b->h_tiles + off;
            sizes[i] = size;
            if (i == 0)
                first = off;
            else if (off != ((end + 15u) & ~15u))
                extent = false;
            rel[i] = off - first;
            end = off + size;
        }
    }
    /* The GPU encoders lay a raster's streams of a strip out as ONE extent in tile order (pass B'): one
     * write appends them all.  (An alias raster of the fused encoder -- its tiles ARE another raster's
     * streams -- points into that raster's extent: the same test holds when every tile is aliased alike;
     * a mixture falls back to gathered writes, 512 tiles per system call.) */
    if (ok && extent)
        ok = gcn10_tiff_put_extent(j->tif, j->b->h_tiles + first, (size_t)(end - first), (int)n, txs, tys, rel, sizes) == 0;
    else if (ok)
        ok = gcn10_tiff_put_tiles(j->tif, (int)n, txs, tys, data, sizes) == 0;
    if (!ok)
        atomic_store(&j->w->failed, true);
    free(txs);
    free(tys);
    free(data);
    free(sizes);
    free(rel);
    gcn10_job_group_done(&j->b->jobs);
    free(j);
}

/* the end of a raster's file: directory, close, rename */
struct finish_job {
    struct worker *w;
    struct strip_buf *b;
    gcn10_tiff_writer *tif;
};

static void finish_tiff_job(void *arg)
{
    struct finish_job *j = arg;
    char err[1024] = "";

    if (gcn10_tiff_finish(j->tif, err, sizeof err) != 0)
        wlog(j->w, "ERROR", true, "%s", err);           /* "write error %d on %s", src/raster.c:221 */
    gcn10_job_group_done(&j->b->jobs);
    free(j);
}

/* One job per strip waits for the strip's compressed bytes to arrive in pinned memory (ONE thread of the pool in
 * hipEventSynchronize instead of one per raster, round 3) and then hands the rasters' extents to the pool. */
struct gate_job {
    struct worker *w;
    struct strip_buf *b;
    gcn10_tiff_writer *tifs[GCN10_N_RASTERS];
    int ty0, across, down;
    long seq;                               /* COG: this strip's turn among the worker's strips */
};

static void strip_gate_job(void *arg)
{
    struct gate_job *g = arg;
    struct run *r = g->w->run;
    const bool arrived = r->gpu->event_sync(g->w->ctx, g->b->ev_d2h) == 0;

    if (!arrived)
        atomic_store(&g->w->failed, true);
    if (r->cog) {
        /* a COG takes its tile data in file order: this strip's extents go after the previous strip's, here on
         * this thread (gate jobs are queued in strip order and the pool is FIFO, so the turn before is running) */
        pthread_mutex_lock(&g->w->gate_mu);
        while (g->w->gate_turn != g->seq)
            pthread_cond_wait(&g->w->gate_cv, &g->w->gate_mu);
        pthread_mutex_unlock(&g->w->gate_mu);
    }
    for (int q = 0; arrived && q < r->n_sel; q++) {       /* stream q of the table = the q-th selected raster */
        struct put_job *j = malloc(sizeof *j);

        if (!j) {
            atomic_store(&g->w->failed, true);
            break;
        }
        *j = (struct put_job){ g->w, g->b, g->tifs[r->sel[q]], q, g->ty0, g->across, g->down };
        gcn10_job_group_add(&g->b->jobs, 1);
        if (r->cog)
            put_tiles_job(j);
        else
            gcn10_pool_submit(r->pool, put_tiles_job, j);
    }
    if (r->cog) {
        pthread_mutex_lock(&g->w->gate_mu);
        g->w->gate_turn++;
        pthread_cond_broadcast(&g->w->gate_cv);
        pthread_mutex_unlock(&g->w->gate_mu);
    }
    gcn10_job_group_done(&g->b->jobs);
    free(g);
}

void gcn10_sink_wait(struct strip_buf *b)
{
    double t0 = now_seconds();

    gcn10_job_group_wait(&b->jobs);
    if (b->owner)
        b->owner->t_sink_wait += now_seconds() - t0;
}

/* hands the finished strip in buffer b to the compression pool */
static int drain_strip_inner(struct worker *w, struct strip_buf *b, gcn10_tiff_writer *tifs[GCN10_N_RASTERS],
                             int W, int H)
{
    struct run *r = w->run;

    if (!b->d2h_issued)
        return 0;
    b->d2h_issued = false;
    if (r->gpu_deflate) {
        /* the sizes are known only now: fetch exactly the bytes the encoder produced */
        const struct gcn10_gpu_api *g = r->gpu;
        int across = (W + TILE - 1) / TILE, down = (b->rows + TILE - 1) / TILE;
        size_t used;

        if (g->event_sync(w->ctx, b->ev_meta) != 0)
            goto gpu_error;
        used = (size_t)*b->h_cursor;
        if (used > b->arena_cap) {
            wlog(w, "ERROR", true, "gpu deflate arena overflow (%zu > %zu)", used, b->arena_cap);
            return -1;
        }
        if (r->null_sink)
            return 0;
        {
            /* CN rasters compress to a few percent, so the pinned arena is an eighth of the
             * worst case; a strip of noise that needs more takes a pageable detour */
            uint8_t *dst = b->h_arena;

            free(b->h_spill);
            b->h_spill = NULL;
            if (used > b->h_arena_cap) {
                b->h_spill = aligned_alloc(4096, (used + 4095) & ~(size_t)4095);
                if (!b->h_spill) {
                    wlog(w, "ERROR", true, "malloc failed for %zu bytes of compressed tiles", used);
                    return -1;
                }
                dst = b->h_spill;
            }
            b->h_tiles = dst;
            b->h_tiles_used = used;
            /* the sink jobs wait for this copy themselves: the worker goes on to the next strip */
            /* (whole 4096-byte units: an O_DIRECT write of the last extent reads up to the next multiple;
             * both arenas are that much larger than `used` can get) */
            if (g->memcpy_d2h(w->ctx, dst, b->d_arena, (used + 4095) & ~(size_t)4095, w->s_d2h) != 0 ||
                g->event_record(w->ctx, b->ev_d2h, w->s_d2h) != 0)
                goto gpu_error;
        }
        {
            struct gate_job *j = malloc(sizeof *j);

            if (!j) {
                wlog(w, "ERROR", true, "malloc failed for tile job");
                return -1;
            }
            j->w = w;
            j->b = b;
            memcpy(j->tifs, tifs, sizeof j->tifs);
            j->ty0 = b->y0 / TILE;
            j->across = across;
            j->down = down;
            j->seq = w->gate_seq++;
            gcn10_job_group_add(&b->jobs, 1);
            gcn10_pool_submit(r->pool, strip_gate_job, j);
        }
        return 0;
gpu_error:
        wlog(w, "ERROR", true, "gpu: %s", g->last_error());
        return -1;
    }
    if (r->gpu->event_sync(w->ctx, b->ev_d2h) != 0) {
        wlog(w, "ERROR", true, "gpu: %s", r->gpu->last_error());
        return -1;
    }
    if (r->null_sink)
        return 0;
    for (int ty = b->y0 / TILE; ty * TILE < b->y0 + b->rows; ty++) {
        for (int q = 0; q < r->n_sel; q++) {
            const int k = r->sel[q];
            struct tile_job *j = malloc(sizeof *j);

            if (!j) {
                wlog(w, "ERROR", true, "malloc failed for tile job");
                return -1;
            }
            *j = (struct tile_job){ w, b, tifs[k], b->h_out[k], W, H, b->y0, ty };
            gcn10_job_group_add(&b->jobs, 1);
            gcn10_pool_submit(r->pool, tile_row_job, j);
        }
    }
    return 0;
}

int gcn10_sink_drain(struct worker *w, struct strip_buf *b, gcn10_tiff_writer *tifs[GCN10_N_RASTERS], int W, int H)
{
    double t0 = now_seconds();
    int rc = drain_strip_inner(w, b, tifs, W, H);

    w->t_gpu_wait += now_seconds() - t0;
    return rc;
}

/* The end of a block's files: directory, close and rename of the 18, side by side on the I/O pool (4 ms per block in a
 * row), with their statistics (stats=1); ok = false: the block was given up and its files go.  Every strip has been
 * drained, so the job counter of the first strip buffer is idle and counts these. */
void gcn10_sink_finish_files(struct worker *w, gcn10_tiff_writer *tifs[GCN10_N_RASTERS], bool ok, int block_id)
{
    struct run *r = w->run;
    struct strip_buf *b0 = &w->buf[0];
    char err[1024] = "";

    for (int k = 0; k < GCN10_N_RASTERS; k++) {
        struct finish_job *j;

        if (!tifs[k])
            continue;
        if (!ok) {
            gcn10_tiff_abort(tifs[k]);
            tifs[k] = NULL;
            continue;
        }
        if (r->stats) {
            /* the raster's exact histogram from the block's pairs, its statistics as GDAL would compute them */
            uint64_t hist[256];
            gcn10_band_stats st;
            char xml[GCN10_STATS_XML_MAX];

            gcn10_raster_histogram((const uint64_t *)w->h_hist, r->hist_codes,
                                   (const int (*)[5])r->tables[k % 9], k < 9, hist);
            gcn10_band_stats_of(hist, r->nodata, &st);
            if (gcn10_tiff_set_metadata_xml(tifs[k], gcn10_stats_xml(&st, xml, sizeof xml) ? xml : NULL) != 0)
                wlog(w, "ERROR", true, "write error: the statistics of block %d raster %d do not fit", block_id, k);
        }
        j = r->pool ? malloc(sizeof *j) : NULL;
        if (!j) {
            if (gcn10_tiff_finish(tifs[k], err, sizeof err) != 0)
                wlog(w, "ERROR", true, "%s", err);      /* "write error %d on %s", src/raster.c:221 */
            tifs[k] = NULL;
            continue;
        }
        *j = (struct finish_job){ w, b0, tifs[k] };
        tifs[k] = NULL;
        gcn10_job_group_add(&b0->jobs, 1);
        gcn10_pool_submit(r->pool, finish_tiff_job, j);
    }
    gcn10_job_group_wait(&b0->jobs);
}

void gcn10_sink_job_cpu(gcn10_pool *pool, struct gcn10_job_cpu by_kind[4])
{
    static const gcn10_job_fn kinds[4] = { put_tiles_job, strip_gate_job, finish_tiff_job, tile_row_job };

    for (int i = 0; i < 4; i++)
        by_kind[i].seconds = gcn10_pool_cpu_of(pool, kinds[i], &by_kind[i].n);
}

/* ---- worker resources ---- */

void gcn10_sink_free_buffers(struct worker *w)
{
    const struct gcn10_gpu_api *g = w->run->gpu;

    for (int i = 0; i < w->run->nbuf; i++) {
        struct strip_buf *b = &w->buf[i];

        for (int k = 0; k < GCN10_N_RASTERS; k++) {
            if (b->h_out[k]) g->host_free(w->ctx, b->h_out[k]);
            if (b->d_out[k]) g->free(w->ctx, b->d_out[k]);
            b->h_out[k] = b->d_out[k] = NULL;
        }
        if (b->h_arena) g->host_free(w->ctx, b->h_arena);
        free(b->h_spill);
        b->h_spill = NULL;
        if (b->d_arena) g->free(w->ctx, b->d_arena);
        if (b->h_table) g->host_free(w->ctx, b->h_table);
        if (b->d_table) g->free(w->ctx, b->d_table);
        if (b->h_cursor) g->host_free(w->ctx, b->h_cursor);
        if (b->d_cursor) g->free(w->ctx, b->d_cursor);
        if (b->d_ptrs) g->free(w->ctx, (void *)b->d_ptrs);
        b->h_arena = b->d_arena = NULL;
        b->h_table = b->d_table = NULL;
        b->h_cursor = b->d_cursor = NULL;
        b->d_ptrs = NULL;
    }
    w->buf_px = 0;
    w->buf_tiles = 0;
}

/* strip buffers sized for blocks W wide: nbuf x (1 + 18) pinned + the same in HBM */
int gcn10_sink_ensure_buffers(struct worker *w, int W)
{
    const struct gcn10_gpu_api *g = w->run->gpu;
    size_t px = (size_t)W * (size_t)w->strip_rows;
    size_t n_tiles = (size_t)((W + TILE - 1) / TILE) * (size_t)(w->strip_rows / TILE);

    if (px <= w->buf_px && n_tiles <= w->buf_tiles)
        return 0;
    gcn10_sink_free_buffers(w);
    for (int i = 0; i < w->run->nbuf; i++) {
        struct strip_buf *b = &w->buf[i];

        for (int q = 0; q < w->run->n_sel; q++) {
            const int k = w->run->sel[q];

            if (!w->run->gpu_deflate)
            {
                GPU_OR_RETURN(w, -1, g->host_alloc(w->ctx, px, (void **)&b->h_out[k]));
                atomic_fetch_add(&w->run->pinned_bytes, (long long)px);
            }
            if (!w->fused && !w->run->aggregate)        /* (an aggregate run makes no full-resolution strip) */
                GPU_OR_RETURN(w, -1, g->malloc(w->ctx, px, (void **)&b->d_out[k]));
        }
        if (w->run->gpu_deflate) {
            size_t tiles = n_tiles;

            b->arena_cap = w->run->lzw ? g->lzw_arena_bound(W, w->strip_rows, GCN10_N_RASTERS)
                                       : g->deflate_arena_bound(W, w->strip_rows, GCN10_N_RASTERS);
            GPU_OR_RETURN(w, -1, g->malloc(w->ctx, b->arena_cap + 4096, (void **)&b->d_arena));
            b->h_arena_cap = b->arena_cap / 8 > ((size_t)32 << 20) ? b->arena_cap / 8 : ((size_t)32 << 20);
            if (getenv("GCN10_PINNED_ARENA_BYTES"))        /* tests: force the spill path */
                b->h_arena_cap = (size_t)strtoull(getenv("GCN10_PINNED_ARENA_BYTES"), NULL, 10);
            if (b->h_arena_cap < 4096)
                b->h_arena_cap = 4096;
            if (b->h_arena_cap > b->arena_cap)
                b->h_arena_cap = b->arena_cap;
            b->h_arena_cap &= ~(size_t)4095;
            GPU_OR_RETURN(w, -1, g->host_alloc(w->ctx, b->h_arena_cap + 4096, (void **)&b->h_arena));
            atomic_fetch_add(&w->run->pinned_bytes, (long long)(b->h_arena_cap + 4096 + tiles * GCN10_N_RASTERS * 8));
            GPU_OR_RETURN(w, -1, g->malloc(w->ctx, tiles * GCN10_N_RASTERS * 8, (void **)&b->d_table));
            GPU_OR_RETURN(w, -1, g->host_alloc(w->ctx, tiles * GCN10_N_RASTERS * 8, (void **)&b->h_table));
            GPU_OR_RETURN(w, -1, g->malloc(w->ctx, 8, (void **)&b->d_cursor));
            GPU_OR_RETURN(w, -1, g->host_alloc(w->ctx, 8, (void **)&b->h_cursor));
            if (!w->fused && !w->run->aggregate) {
                /* the per-raster encoder takes the selected strips, packed in raster order */
                uint8_t *packed[GCN10_N_RASTERS] = { 0 };

                for (int q = 0; q < w->run->n_sel; q++)
                    packed[q] = b->d_out[w->run->sel[q]];
                GPU_OR_RETURN(w, -1, g->malloc(w->ctx, GCN10_N_RASTERS * sizeof(void *), (void **)&b->d_ptrs));
                GPU_OR_RETURN(w, -1, g->memcpy_h2d(w->ctx, (void *)b->d_ptrs, packed, GCN10_N_RASTERS * sizeof(void *),
                                         w->s_kernel));
                GPU_OR_RETURN(w, -1, g->stream_sync(w->ctx, w->s_kernel));
            }
        }
    }
    w->buf_px = px;
    w->buf_tiles = n_tiles;
    return 0;
}

int gcn10_ensure_pinned_on(struct worker *w, gcn10_gpu_ctx *ctx, void **p, size_t *cap, size_t need)
{
    const struct gcn10_gpu_api *g = w->run->gpu;

    if (need <= *cap)
        return 0;
    if (*p)
        g->host_free(ctx, *p);
    *p = NULL;
    *cap = 0;
    need += need / 8 + 4096;
    GPU_OR_RETURN(w, -1, g->host_alloc(ctx, need, p));
    atomic_fetch_add(&w->run->pinned_bytes, (long long)need);
    *cap = need;
    return 0;
}

int gcn10_ensure_dev_on(struct worker *w, gcn10_gpu_ctx *ctx, void **p, size_t *cap, size_t need)
{
    const struct gcn10_gpu_api *g = w->run->gpu;

    if (need <= *cap)
        return 0;
    if (*p)
        GPU_OR_RETURN(w, -1, g->free(ctx, *p));
    *p = NULL;
    *cap = 0;
    GPU_OR_RETURN(w, -1, g->malloc(ctx, need, p));
    *cap = need;
    return 0;
}
