/* pipeline.c -- the workers of a run (run.c) and the per-block pipeline.
 *
 * What the reference does per block on one MPI rank
 * (src/cn.c:134-384): find the block's bbox, load the
 * landcover window and the soil window with GDAL, upsample, then 18 times
 * {read CSV, memcpy, remap, memset, lookup, GDAL DEFLATE write}.
 *
 * Here, per block, two threads per GPU worker:
 *   input  (pipeline_input.c, one block AHEAD): bbox -> windows (geo.c, bit-exact) -> soil window +
 *          index maps -> HBM; the landcover window's chunks as they lie in the files -> pinned ring ->
 *          HBM -> decoded / untiled there into the row-major block
 *   encode (here): per strip of rows ONE fused device pass turns landcover + soil into the compressed
 *          256x256 tiles of all 18 rasters (no CN raster in HBM); the tiles of a raster and a strip are
 *          one extent of the arena, copied back on the d2h stream into pinned memory; buffer sets rotate,
 *          so kernels, copy-back and file writes of neighbouring strips overlap
 *   sink   (sink.c) one write per raster and strip appends the extent to the raster's GeoTIFF (I/O pool)
 * Blocks are pulled from one atomic counter by all workers (the reference's
 * static `i += size` round-robin, src/main.c:171, made dynamic); no data moves
 * between GPUs, so there is no collective and no RCCL.
 */
#include "pipeline_internal.h"

#include <errno.h>
#include <limits.h>
#include <sched.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>

double gcn10_now_seconds(void)
{
    struct timespec ts;

    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

void gcn10_wlog(struct worker *w, const char *level, bool console, const char *fmt, ...)
{
    char msg[8192];                         /* char msg[8192], src/cn.c:144 */
    va_list ap;

    va_start(ap, fmt);
    vsnprintf(msg, sizeof msg, fmt, ap);
    va_end(ap);
    gcn10_log_message(w->log, level, msg, console);
}

#define now_seconds gcn10_now_seconds
#define wlog gcn10_wlog

/* ------------------------------------------------------------------------ */
/* one block: src/cn.c:134-384                                               */
/* ------------------------------------------------------------------------ */

/* output path with the reference's non-overwrite rule: an existing file is left
 * alone and the new one gets a trailing underscore (src/cn.c:320-360) */
static void output_path(char *out, size_t cap, const struct run *r, const char *cond, const char *hc, const char *arc,
                        int block_id, bool overwrite)
{
    /* cn_rasters_<cond>/cn_<hc>_<arc>_<id>.tif, src/cn.c:308 */
    snprintf(out, cap, "%s_%s%s/%s_%s_%s_%d.tif", r->out_dir, cond, r->out_suffix, r->out_name, hc, arc, block_id);
    if (!overwrite) {
        FILE *f = fopen(out, "r");

        if (f) {
            fclose(f);
            snprintf(out, cap, "%s_%s%s/%s_%s_%s_%d_.tif", r->out_dir, cond, r->out_suffix, r->out_name, hc, arc,
                     block_id);                                                                 /* :341 */
        }
    }
}

/* overview levels of a COG block; a window that would need more than GCN10_COG_MAX_LEVELS gets none here (the
 * encoder refuses the block) */
static int cog_levels_of(int W, int H)
{
    int L = gcn10_cog_levels(W, H);

    return L > GCN10_COG_MAX_LEVELS ? 0 : L;
}

/* output directories (src/cn.c:237-256) and the files of the run's rasters, for block `in` */
int gcn10_create_outputs(struct worker *w, struct block_in *in)
{
    struct run *r = w->run;
    char err[1024] = "";
    double t_mark = now_seconds();

    if (r->null_sink) {
        in->tifs_ok = true;
        return 0;
    }
    for (int c = 0; c < 2; c++) {
        char dir[64];

        if (!(r->cond_mask & (1u << c)))
            continue;
        snprintf(dir, sizeof dir, "%s_%s%s", r->out_dir, gcn10_conds[c], r->out_suffix);
        if (mkdir(dir, 0755) != 0 && errno != EEXIST) {
            wlog(w, "ERROR", true, "failed to create output directory %s", dir);       /* src/cn.c:250 */
            return -1;
        }
    }
    for (int q = 0; q < r->n_sel; q++) {
        const int k = r->sel[q];
        char path[PATH_MAX];

        output_path(path, sizeof path, r, gcn10_conds[k / 9], gcn10_hcs[(k % 9) / 3], gcn10_arcs[k % 3], in->block_id,
                    r->opt.overwrite);
        if (r->cog)
            in->tifs[k] = gcn10_tiff_create_cog(path, in->W, in->H, in->gt, gcn10_raster_georef(w->esa),
                                                cog_levels_of(in->W, in->H), err, sizeof err);
        else
            in->tifs[k] = gcn10_tiff_create(path, in->out_W, in->out_H, in->out_gt, gcn10_raster_georef(w->esa), err,
                                            sizeof err);
        if (!in->tifs[k]) {
            wlog(w, "ERROR", true, "%s", err);          /* save_raster logs and goes on, src/raster.c:220-223 */
            gcn10_abort_outputs(in);
            w->t_create += now_seconds() - t_mark;
            return 1;
        }
        if (r->lzw)
            (void)gcn10_tiff_set_compression(in->tifs[k], 5);
        /* before any tile: a COG lays its directories out with these tags (the statistics come at finish) */
        if ((r->nodata >= 0 && gcn10_tiff_set_nodata(in->tifs[k], r->nodata) != 0) ||
            (r->stats && gcn10_tiff_reserve_metadata(in->tifs[k], GCN10_STATS_XML_MAX) != 0)) {
            wlog(w, "ERROR", true, "write error: cannot place the GDAL tags of %s", path);
            gcn10_abort_outputs(in);
            w->t_create += now_seconds() - t_mark;
            return 1;
        }
        if (r->direct_io && r->gpu_deflate)
            gcn10_tiff_set_direct(in->tifs[k], true);   /* best effort: a file system that refuses writes buffered */
    }
    in->tifs_ok = true;
    w->t_create += now_seconds() - t_mark;
    return 0;
}

void gcn10_abort_outputs(struct block_in *in)
{
    for (int k = 0; k < GCN10_N_RASTERS; k++) {
        if (in->tifs[k])
            gcn10_tiff_abort(in->tifs[k]);
        in->tifs[k] = NULL;
    }
    in->tifs_ok = false;
}

/* The strips of one raster (a block, or a level of its overviews) through the encoder and the sink.  d_block / d_cj:
 * its landcover and soil rows, for the prepared tile of width W.  premade (device, [strip][GCN10_N_RASTERS]): the
 * selected rasters are already made (average overviews, aggregated rasters), strip s's n_sel pointers at
 * premade + s * GCN10_N_RASTERS, and only the per-raster encoder runs.  hist (device, stats=1, the block's own strips only): every strip's
 * (landcover, soil code) pairs are added to it, behind the strip's encoder on the same stream.  Every strip has been
 * handed to the sink, and the sink is done, on return.  0, or -1 (logged) for errors the reference answers with
 * MPI_Abort. */
int gcn10_run_strips(struct worker *w, int W, int H, const uint8_t *d_block, const int32_t *d_cj,
                     const uint8_t *const *premade, unsigned long long *hist, gcn10_tiff_writer *tifs[GCN10_N_RASTERS])
{
    struct run *r = w->run;
    const struct gcn10_gpu_api *g = r->gpu;
    int n_strips;

    /* strips: rows are multiples of 256 (whole GeoTIFF tile rows) and of 16
     * (16-byte aligned strip starts for any W) */
    n_strips = (H + w->strip_rows - 1) / w->strip_rows;

    for (int s = 0; s < n_strips; s++) {
        struct strip_buf *b = &w->buf[s % r->nbuf];
        int y0 = s * w->strip_rows;
        int rows = H - y0 < w->strip_rows ? H - y0 : w->strip_rows;
        size_t px = (size_t)W * (size_t)rows;
        uint8_t *outs[GCN10_N_RASTERS];
        const uint8_t *d_esa = d_block ? d_block + (size_t)y0 * (size_t)W : NULL;

        /* this buffer's previous strip: its D2H must be done and handed to the sink,
         * and the sink must be done with the pinned buffers */
        if (gcn10_sink_drain(w, b, tifs, W, H) != 0)
            return -1;
        gcn10_sink_wait(b);

        /* the strip's kernels on the compute stream */
        if (premade) {
            if ((r->lzw ? g->lzw_strip : g->deflate_strip)(w->ctx, premade + (size_t)s * GCN10_N_RASTERS, r->n_sel, W,
                                                           rows, b->d_arena, b->arena_cap, b->d_table, b->d_cursor,
                                                           w->s_kernel) != 0)
                goto gpu_fail;
        }
        else if (w->fused) {
            /* landcover + soil -> 18 x compressed tiles in one device pass, no CN strip in HBM */
            if (g->deflate_fused_strip(w->ctx, d_esa, W, rows, d_cj + y0, r->cond_mask, r->table_mask, b->d_arena,
                                       b->arena_cap, b->d_table, b->d_cursor, w->s_kernel) != 0)
                goto gpu_fail;
        }
        else {
            for (int k = 0; k < GCN10_N_RASTERS; k++)
                outs[k] = b->d_out[k];             /* NULL for a raster this run does not produce */
            /* (a runoff_rain run: every value through the byte table of the pixel's rain cell) */
            if ((w->runoff ? g->runoff_strip(w->ctx, d_esa, W, rows, d_cj + y0, w->runoff->d_cellx,
                                             w->runoff->d_celly + y0, w->runoff->ncx, w->runoff->ncy,
                                             w->runoff->d_cells, r->cond_mask, r->table_mask, outs, w->s_kernel)
                           : g->cn_strip(w->ctx, d_esa, W, rows, d_cj + y0, r->cond_mask, r->table_mask, outs,
                                         w->s_kernel)) != 0)
                goto gpu_fail;
            /* encode the selected strips where they are */
            if (r->gpu_deflate &&
                (r->lzw ? g->lzw_strip : g->deflate_strip)(w->ctx, b->d_ptrs, r->n_sel, W, rows, b->d_arena,
                                                           b->arena_cap, b->d_table, b->d_cursor, w->s_kernel) != 0)
                goto gpu_fail;
        }
        if (g->event_record(w->ctx, b->ev_kernel, w->s_kernel) != 0 ||
            g->stream_wait_event(w->ctx, w->s_d2h, b->ev_kernel) != 0)
            goto gpu_fail;
        /* the statistics' counts after the event: the strip's copy-back does not wait for them */
        if (hist && g->pair_histogram(w->ctx, d_esa, W, rows, d_cj + y0, hist, w->s_kernel) != 0)
            goto gpu_fail;
        /* ... and what comes back on the copy stream */
        if (r->gpu_deflate) {
            /* sizes and offsets now; the compressed bytes when drain_strip knows how many */
            int across = (W + TILE - 1) / TILE, down = (rows + TILE - 1) / TILE;

            if (g->memcpy_d2h(w->ctx, b->h_cursor, b->d_cursor, 8, w->s_d2h) != 0 ||
                g->memcpy_d2h(w->ctx, b->h_table, b->d_table,
                              (size_t)across * down * (size_t)r->n_sel * 8, w->s_d2h) != 0 ||
                g->event_record(w->ctx, b->ev_meta, w->s_d2h) != 0)
                goto gpu_fail;
        }
        else {
            for (int q = 0; q < r->n_sel; q++)
                if (g->memcpy_d2h(w->ctx, b->h_out[r->sel[q]], b->d_out[r->sel[q]], px, w->s_d2h) != 0)
                    goto gpu_fail;
            if (g->event_record(w->ctx, b->ev_d2h, w->s_d2h) != 0)
                goto gpu_fail;
        }
        b->d2h_issued = true;
        b->y0 = y0;
        b->rows = rows;

        /* While this strip is in flight, hand an earlier one to the sink: the one `drain_lag` strips back
         * (default 2).  Draining waits for that strip's kernels and counts; with a lag of 1 (rounds 1-2) the
         * worker had exactly one strip queued behind the running one and could submit the next only when the
         * previous had finished -- the trace of round 3 shows the compute stream idle ~0.5 ms between strips
         * whose kernels take 0.2-0.3 ms.  With 2 the queue holds two strips while the host waits. */
        if (s >= r->drain_lag && gcn10_sink_drain(w, &w->buf[(s - r->drain_lag) % r->nbuf], tifs, W, H) != 0)
            return -1;
    }
    if (r->cog) {
        /* a COG's strips reach the sink in strip order */
        for (int s = n_strips > r->nbuf ? n_strips - r->nbuf : 0; s < n_strips; s++)
            if (gcn10_sink_drain(w, &w->buf[s % r->nbuf], tifs, W, H) != 0)
                return -1;
    }
    for (int i = 0; i < w->run->nbuf; i++)
        if (gcn10_sink_drain(w, &w->buf[i], tifs, W, H) != 0)
            return -1;
    for (int i = 0; i < w->run->nbuf; i++)
        gcn10_sink_wait(&w->buf[i]);
    return 0;

gpu_fail:
    wlog(w, "ERROR", true, "gpu: %s", g->last_error());
    return -1;
}

/* The overview phase of a COG block (levels L .. 1, smallest first): made on the GPU, encoded by the run's encoders,
 * appended to the files before any full-resolution tile.  nearest: every level is a block of its own -- its
 * landcover gathered from the block's, its soil index maps the block's composed with the same sampling -- through
 * prepare_tile and the strip encoder of the run; the block's own tile is prepared again afterwards.  average: the
 * whole pyramid of the selected rasters from landcover + soil in one pass per strip (gcn10_gpu_overview_average on
 * the block's prepared tile), then every level through the per-raster encoder.  0, or -1 (logged). */
static int encode_overviews(struct worker *w, struct block_in *in, gcn10_tiff_writer *tifs[GCN10_N_RASTERS], int L)
{
    struct run *r = w->run;
    const struct gcn10_gpu_api *g = r->gpu;
    const int W = in->W, H = in->H;
    gcn10_tiff_writer *lv[GCN10_N_RASTERS];

    if (!r->ov_average) {
        for (int k = L; k >= 1; k--) {
            const int32_t *d_cj;
            int Wk, Hk;

            if (gcn10_level_nearest(w, in, k, &Wk, &Hk, &d_cj) != 0)
                return -1;
            for (int q = 0; q < GCN10_N_RASTERS; q++)
                lv[q] = tifs[q] ? gcn10_tiff_level(tifs[q], k) : NULL;
            if (gcn10_run_strips(w, Wk, Hk, w->d_ov, d_cj, NULL, NULL, lv) != 0)
                return -1;
            /* the next level overwrites the index maps and the level's landcover: this one's kernels are done */
            GPU_OR_RETURN(w, -1, g->stream_sync(w->ctx, w->s_kernel));
        }
        GPU_OR_RETURN(w, -1, g->prepare_tile(w->ctx, in->d_coarse, in->hsx, in->hsy, in->d_ci, W, w->s_kernel));
        return 0;
    }

    /* average: the pyramid of the selected rasters, level by level, raster by raster */
    {
        uint8_t *levels[GCN10_N_RASTERS * GCN10_COG_MAX_LEVELS];
        /* level 1 has the most strips */
        const size_t n_ptrs = ((size_t)gcn10_level_dim(H, 1) + (size_t)w->strip_rows - 1) / (size_t)w->strip_rows;

        if (gcn10_ensure_dev_on(w, w->ctx, &w->d_ov_ptrs, &w->ov_ptrs_cap, n_ptrs * GCN10_N_RASTERS * sizeof(void *)) != 0 ||
            gcn10_levels_average(w, in, L, w->strip_rows, levels) != 0)
            return -1;
        for (int k = L; k >= 1; k--) {
            const int Wk = gcn10_level_dim(W, k), Hk = gcn10_level_dim(H, k);
            const int n_strips = (Hk + w->strip_rows - 1) / w->strip_rows;
            const uint8_t **tab = calloc((size_t)n_strips * GCN10_N_RASTERS, sizeof *tab);

            if (!tab) {
                wlog(w, "ERROR", true, "malloc failed for overview strips");
                return -1;
            }
            for (int s = 0; s < n_strips; s++)
                for (int q = 0; q < r->n_sel; q++)
                    tab[(size_t)s * GCN10_N_RASTERS + q] =
                        levels[q * L + k - 1] + (size_t)s * (size_t)w->strip_rows * (size_t)Wk;
            if (g->memcpy_h2d(w->ctx, w->d_ov_ptrs, tab, (size_t)n_strips * GCN10_N_RASTERS * sizeof *tab,
                              w->s_kernel) != 0 ||
                g->stream_sync(w->ctx, w->s_kernel) != 0) {
                wlog(w, "ERROR", true, "gpu: %s", g->last_error());
                free(tab);
                return -1;
            }
            free(tab);
            for (int q = 0; q < GCN10_N_RASTERS; q++)
                lv[q] = tifs[q] ? gcn10_tiff_level(tifs[q], k) : NULL;
            if (gcn10_run_strips(w, Wk, Hk, NULL, NULL, (const uint8_t *const *)w->d_ov_ptrs, NULL, lv) != 0)
                return -1;
            GPU_OR_RETURN(w, -1, g->stream_sync(w->ctx, w->s_kernel));    /* the pointer table is rewritten next */
        }
    }
    return 0;
}

int gcn10_block_statuses(struct worker *w, const struct block_in *in)
{
    if (in->n_inflate == 0)
        return GCN10_BLOCK_READY;
    /* every landcover chunk must have been a valid one (the statuses came back behind ev_ready) */
    if (w->run->gpu->event_sync(w->ctx, in->ev_ready) != 0)
        return GCN10_BLOCK_DEVICE_ERROR;
    for (size_t i = 0; i < in->n_inflate; i++)
        if (in->jl.h_status[i] != 0) {
            wlog(w, "ERROR", true, "gdalrasterio error: cannot decode a tile of the window %d,%d %dx%d "
                                   "(stream %zu, reason %u)", in->xoff, in->yoff, in->W, in->H, i, in->jl.h_status[i]);
            wlog(w, "ERROR", true, "esa load failed for block %d", in->block_id);
            return GCN10_BLOCK_UNREADABLE;
        }
    return GCN10_BLOCK_READY;
}

int gcn10_block_take(struct worker *w, const struct block_in *in)
{
    if (w->run->gpu->stream_wait_event(w->ctx, w->s_kernel, in->ev_ready) != 0)
        return GCN10_BLOCK_DEVICE_ERROR;
    return gcn10_block_statuses(w, in);
}

/* The back half of process_block (src/cn.c:236-384) for a block whose input the input side has put on its
 * way to HBM.  Returns 0 (done, or skipped like the reference skips) or -1 for errors the
 * reference answers with MPI_Abort */
int gcn10_encode_block(struct worker *w, struct block_in *in)
{
    struct run *r = w->run;
    const struct gcn10_gpu_api *g = r->gpu;
    const int W = in->W, H = in->H, block_id = in->block_id;
    gcn10_tiff_writer *tifs[GCN10_N_RASTERS] = { 0 };
    int rc = 0;
    bool ok = false;
    double t_mark = now_seconds();
    /* COG: the block's overview levels; nearest ones are encoded as blocks of their own (encode_overviews) */
    const int L = r->cog ? gcn10_cog_levels(W, H) : 0;
    const bool nearest_levels = r->cog && !r->ov_average && L > 0 && L <= GCN10_COG_MAX_LEVELS;

    if (getenv("GCN10_TEST_FAIL_BLOCK") && atoi(getenv("GCN10_TEST_FAIL_BLOCK")) == block_id) {
        /* test hook (tools/r03/run_rehearse_8gpu.sh): one worker meets an error of the kind the reference answers
         * with MPI_Abort -- the whole run must stop and exit with code 1 (src/main.c:175, src/cn.c:25, 216) */
        wlog(w, "ERROR", true, "malloc failed for block %d (GCN10_TEST_FAIL_BLOCK)", block_id);
        return -1;
    }
    /* the 18 files were created by the input side (gcn10_create_outputs), one block ahead */
    memcpy(tifs, in->tifs, sizeof tifs);
    memset(in->tifs, 0, sizeof in->tifs);
    if (!r->null_sink && !in->tifs_ok)
        goto out;                       /* save_raster logs and goes on, src/raster.c:220-223: logged at creation */
    t_mark = now_seconds();

    /* device side of the block: the encoder waits (on the device) for the input side's copies and kernels */
    w->strip_rows = r->strip_rows;
    if (gcn10_sink_ensure_buffers(w, in->out_W) != 0) {
        rc = -1;
        goto out;
    }
    atomic_store(&w->failed, false);
    /* nearest overviews prepare their levels' tiles first and the block's after them (encode_overviews); every
     * other block -- average overviews, no levels (a window of at most 256 px), a refused one -- is prepared here */
    if (g->stream_wait_event(w->ctx, w->s_kernel, in->ev_ready) != 0 ||
        (!nearest_levels &&
         g->prepare_tile(w->ctx, in->d_coarse, in->hsx, in->hsy, in->d_ci, W, w->s_kernel) != 0)) {
        wlog(w, "ERROR", true, "gpu: %s", g->last_error());
        rc = -1;
        goto out;
    }
    w->t_device += now_seconds() - t_mark;

    if (r->cog) {
        if (!atomic_exchange(&r->cog_logged, true))
            wlog(w, "INFO", true, "cog: Cloud Optimized GeoTIFFs, overviews by %s resampling, %d levels (block %d, "
                 "%dx%d)", r->ov_average ? "average" : "nearest", L, block_id, W, H);
        if (L > GCN10_COG_MAX_LEVELS) {
            wlog(w, "ERROR", true, "cog: block %d (%dx%d) would need %d overview levels, more than %d: block skipped",
                 block_id, W, H, L, GCN10_COG_MAX_LEVELS);
            goto out;
        }
        if (L > 0 && encode_overviews(w, in, tifs, L) != 0) {
            rc = -1;
            goto out;
        }
    }
    if (r->stats &&
        (gcn10_ensure_dev_on(w, w->ctx, (void **)&w->d_hist, &w->d_hist_cap,
                             GCN10_PAIR_HIST_SIZE * sizeof *w->d_hist) != 0 ||
         gcn10_ensure_pinned_on(w, w->ctx, (void **)&w->h_hist, &w->h_hist_cap,
                                GCN10_PAIR_HIST_SIZE * sizeof *w->h_hist) != 0)) {
        rc = -1;
        goto out;
    }
    if (r->stats && g->memset(w->ctx, w->d_hist, 0, GCN10_PAIR_HIST_SIZE * sizeof *w->d_hist, w->s_kernel) != 0)
        goto gpu_fail;
    if (r->mode->strips(w, in, tifs) != 0) {
        rc = -1;
        goto out;
    }
    if (r->stats &&
        (g->memcpy_d2h(w->ctx, w->h_hist, w->d_hist, GCN10_PAIR_HIST_SIZE * sizeof *w->h_hist, w->s_kernel) != 0 ||
         g->stream_sync(w->ctx, w->s_kernel) != 0))
        goto gpu_fail;
    ok = !atomic_load(&w->failed);
    /* the statuses here, behind the strips, so that decode and encode overlap */
    switch (gcn10_block_statuses(w, in)) {
    case GCN10_BLOCK_DEVICE_ERROR:
        goto gpu_fail;
    case GCN10_BLOCK_UNREADABLE:
        ok = false;
    }
    goto out;

gpu_fail:
    wlog(w, "ERROR", true, "gpu: %s", g->last_error());
    rc = -1;

out:
    /* nothing of this block may still be in flight when its buffers are reused */
    for (int i = 0; i < w->run->nbuf; i++) {
        if (w->buf[i].d2h_issued) {
            g->event_sync(w->ctx, r->gpu_deflate ? w->buf[i].ev_meta : w->buf[i].ev_d2h);
            w->buf[i].d2h_issued = false;
        }
        gcn10_sink_wait(&w->buf[i]);
    }
    if (rc != 0 && w->ctx)
        g->device_sync(w->ctx);
    else if (!ok && w->ctx)
        g->stream_sync(w->ctx, w->s_kernel);    /* a block given up half-way: its kernels may still be queued */
    t_mark = now_seconds();
    gcn10_sink_finish_files(w, tifs, ok, block_id);
    w->t_finish += now_seconds() - t_mark;
    if (ok) {
        for (int q = 0; q < r->n_sel; q++) {
            const int k = r->sel[q];
            /* src/cn.c:366-373: one completion line and one progress line per raster */
            wlog(w, "INFO", false, "completed condition for %d: %s/%s/%s", block_id, gcn10_conds[k / 9],
                 gcn10_hcs[(k % 9) / 3], gcn10_arcs[k % 3]);
            {
                char line[256];

                snprintf(line, sizeof line, "progress: completed block %d / total %d", block_id,
                         r->n_blocks);                                  /* src/log.c:203-206 */
                gcn10_log_message(r->workers[0].log, "INFO", line, false);
            }
        }
    }
    return rc;
}

/* the write run: the block's own strips, counted for the statistics on their way */
static int write_strips(struct worker *w, struct block_in *in, gcn10_tiff_writer *tifs[GCN10_N_RASTERS])
{
    return gcn10_run_strips(w, in->W, in->H, in->d_block, in->d_cj, NULL, w->run->stats ? w->d_hist : NULL, tifs);
}

const struct gcn10_mode gcn10_mode_write = { .writes_block_files = true, .block = gcn10_encode_block,
                                             .strips = write_strips };

/* ------------------------------------------------------------------------ */
/* workers: the ranks of src/main.c:58-203                                   */
/* ------------------------------------------------------------------------ */

static void worker_teardown(struct worker *w)
{
    const struct gcn10_gpu_api *g = w->run->gpu;

    gcn10_input_teardown(w);
    if (w->ctx) {
        g->device_sync(w->ctx);
        if (w->run->mode->worker_teardown)
            w->run->mode->worker_teardown(w);
        gcn10_sink_free_buffers(w);
        for (int i = 0; i < w->run->nbuf; i++) {
            struct strip_buf *b = &w->buf[i];

            if (b->ev_h2d) g->event_destroy(w->ctx, b->ev_h2d);
            if (b->ev_kernel) g->event_destroy(w->ctx, b->ev_kernel);
            if (b->ev_d2h) g->event_destroy(w->ctx, b->ev_d2h);
            if (b->ev_meta) g->event_destroy(w->ctx, b->ev_meta);
        }
        if (w->d_ov) g->free(w->ctx, w->d_ov);
        if (w->d_ov_idx) g->free(w->ctx, w->d_ov_idx);
        if (w->d_ov_ptrs) g->free(w->ctx, w->d_ov_ptrs);
        if (w->d_hist) g->free(w->ctx, w->d_hist);
        if (w->h_hist) g->host_free(w->ctx, w->h_hist);
        w->d_hist = w->h_hist = NULL;
        w->d_hist_cap = w->h_hist_cap = 0;
        w->d_ov = NULL;
        w->d_ov_idx = NULL;
        w->d_ov_ptrs = NULL;
        if (w->s_kernel) g->stream_destroy(w->ctx, w->s_kernel);
        if (w->s_d2h) g->stream_destroy(w->ctx, w->s_d2h);
        g->destroy(w->ctx);
        w->ctx = NULL;
    }
    gcn10_raster_close(w->esa);
    gcn10_raster_close(w->soil);
    w->esa = w->soil = NULL;
    for (int i = 0; i < w->run->nbuf; i++)
        gcn10_job_group_destroy(&w->buf[i].jobs);
    pthread_mutex_destroy(&w->gate_mu);
    pthread_cond_destroy(&w->gate_cv);
}

/* Keeps a worker thread (and the pinned buffers it is about to allocate: first touch)
 * on the NUMA node its GPU hangs off.  Best effort: any failure leaves the thread alone. */
static void bind_to_gpu_numa_node(struct worker *w, int device)
{
    char bus[64] = "", path[256], line[4096];
    FILE *f;
    int node = -1;
    cpu_set_t set;
    char *p;

    w->device = device;
    w->numa_node = -1;
    if (w->run->gpu->pci_bus_id(device, bus, sizeof bus) != 0)
        return;
    for (char *c = bus; *c; c++)
        if (*c >= 'A' && *c <= 'F')
            *c = (char)(*c - 'A' + 'a');        /* sysfs names are lower case */
    snprintf(w->pci_bus, sizeof w->pci_bus, "%s", bus);
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
    f = fopen(path, "r");
    if (!f)
        return;
    if (fscanf(f, "%d", &node) != 1)
        node = -1;
    fclose(f);
    w->numa_node = node;
    if (node < 0 || getenv("GCN10_NO_NUMA_BIND"))
        return;
    snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    f = fopen(path, "r");
    if (!f)
        return;
    if (!fgets(line, sizeof line, f)) {
        fclose(f);
        return;
    }
    fclose(f);
    CPU_ZERO(&set);
    for (p = line; *p;) {                       /* "0-31,64-95" */
        char *end;
        long a = strtol(p, &end, 10), b;

        if (end == p)
            break;
        b = a;
        if (*end == '-') {
            p = end + 1;
            b = strtol(p, &end, 10);
        }
        for (long c = a; c <= b && c < CPU_SETSIZE; c++)
            CPU_SET((int)c, &set);
        p = (*end == ',') ? end + 1 : end;
        if (*end != ',')
            break;
    }
    if (CPU_COUNT(&set) > 0 && sched_setaffinity(0, sizeof set, &set) == 0)
        wlog(w, "INFO", false, "gpu %d (%s) is on NUMA node %d: worker bound to its %d cpus", device, bus,
             node, CPU_COUNT(&set));
}

static int worker_setup(struct worker *w)
{
    struct run *r = w->run;
    const struct gcn10_gpu_api *g = r->gpu;
    char err[1024];

    for (int i = 0; i < w->run->nbuf; i++) {
        gcn10_job_group_init(&w->buf[i].jobs);
        w->buf[i].owner = w;
    }
    pthread_mutex_init(&w->gate_mu, NULL);
    pthread_cond_init(&w->gate_cv, NULL);
    bind_to_gpu_numa_node(w, (w->index % r->n_devices) % r->n_physical);
    if (g->init(w->device, &w->ctx) != 0) {
        wlog(w, "ERROR", true, "gpu %d: %s", w->device, g->last_error());
        return -1;
    }
    {
        char name[128];
        size_t hbm = 0;
        int cus = g->device_info(w->ctx, name, sizeof name, &hbm);

        w->n_cus = cus > 0 ? cus : 256;
    }
    /* waits for GPU events sleep between queries: the pool threads that wait for a strip's bytes, and this thread when
     * it waits for a strip's table, would otherwise spin in user mode for the whole wait (GCN10_EVENT_SLEEP_US=0: spin) */
    if (r->event_sleep_us > 0 && g->set_option)
        (void)g->set_option(w->ctx, "event_sync_sleep_us", r->event_sleep_us);
    GPU_OR_RETURN(w, -1, g->set_tables(w->ctx, &r->tables[0][0][0], 9));
    w->fused = r->fused && g->deflate_fused_available(w->ctx) == 1;
    if (r->fused && !w->fused)
        wlog(w, "INFO", false, "the lookup tables define more than 256 pixel classes: "
                               "per-raster GPU encoding instead of the fused encoder");
    GPU_OR_RETURN(w, -1, g->stream_create(w->ctx, &w->s_kernel));
    GPU_OR_RETURN(w, -1, g->stream_create(w->ctx, &w->s_d2h));
    for (int i = 0; i < w->run->nbuf; i++) {
        GPU_OR_RETURN(w, -1, g->event_create(w->ctx, &w->buf[i].ev_h2d));
        GPU_OR_RETURN(w, -1, g->event_create(w->ctx, &w->buf[i].ev_kernel));
        GPU_OR_RETURN(w, -1, g->event_create(w->ctx, &w->buf[i].ev_d2h));
        GPU_OR_RETURN(w, -1, g->event_create(w->ctx, &w->buf[i].ev_meta));
    }
    /* the reference reopens both rasters for every block (src/raster.c:119);
     * here each worker keeps its own handles */
    w->esa = gcn10_raster_open(r->cfg.esa_data_path, r->cfg.esa_tile_dir, err, sizeof err);
    if (!w->esa)
        wlog(w, "ERROR", true, "%s", err);              /* "gdal open failed: ..." */
    w->soil = gcn10_raster_open(r->cfg.hysogs_data_path, NULL, err, sizeof err);
    if (!w->soil)
        wlog(w, "ERROR", true, "%s", err);
    /* the input side: its own context and stream on the same device, and (prefetch_blocks=1) its thread */
    if (gcn10_input_setup(w) != 0 || gcn10_input_start(w) != 0)
        return -1;
    return 0;
}

void *gcn10_worker_main(void *arg)
{
    struct worker *w = arg;
    struct run *r = w->run;

    if (worker_setup(w) != 0) {
        atomic_store(&r->fatal, 1);
        worker_teardown(w);
        return NULL;
    }
    for (;;) {
        /* the next block of THIS worker: staged one block ahead by its input thread, which takes the ids
         * from the run's counter (the reference's `i += size`, src/main.c:171, made dynamic) */
        struct block_in *in = gcn10_input_next(w);
        double t0;

        if (!in)
            break;
        t0 = now_seconds();
        if (in->outcome == 1 && r->mode->block_unreadable)
            r->mode->block_unreadable(w, in->block_id);
        if (in->outcome == 0 && !atomic_load(&r->fatal) && r->mode->block(w, in) != 0)
            atomic_store(&r->fatal, 1);     /* where the reference calls MPI_Abort */
        gcn10_abort_outputs(in);            /* files of a block that was not encoded after all (a no-op otherwise) */
        w->busy_seconds += now_seconds() - t0;
        w->blocks_done += in->outcome >= 0 ? 1 : 0;
        w->in_seq++;
        /* steady state of this worker: from the end of its first block (buffers allocated and pinned, kernels
         * loaded, workspaces grown) to the end of its last */
        if (w->in_seq == 1)
            w->t_first_done = now_seconds();
        w->t_last_done = now_seconds();
        gcn10_input_release(w, in);
        if (atomic_load(&r->fatal))
            break;
    }
    worker_teardown(w);
    w->cpu_seconds = gcn10_thread_cpu_seconds();
    return NULL;
}
