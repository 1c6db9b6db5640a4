/* aggregate.c -- area-mean CN rasters on a coarser grid (config key "aggregate", --aggregate <f>): no counterpart in
 * the reference.
 *
 * An aggregate run writes no 10 m raster.  Every block is staged as for a write run (input thread, GPU inflate,
 * prepare_tile); the input side also works out the block's grid of f x f pixel cells over its OWNED pixels
 * (gcn10_aggregate_geometry) and creates the files on that grid, cn_rasters_<cond>_x<f>/cn_<hc>_<arc>_<id>.tif.  The
 * worker runs gcn10_gpu_aggregate over the decoded landcover into one small device raster per selected raster -- in
 * ONE band, the block's owned rows: a call's workgroups fill the device only when there are many of them, and bands of
 * a strip's rows cost a third more (DESIGN.md "Aggregated rasters") --, and hands those to the run's per-raster tile
 * encoder and the sink exactly as the average overview levels are (gcn10_run_strips with premade rasters): same
 * arena, table, cursor and spill rules, same writer.  The device rasters live in the worker's overview buffers,
 * which an aggregate run does not use otherwise.
 */
#include "pipeline_internal.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define wlog gcn10_wlog

int gcn10_aggregate_geometry(int W, int H, const double gt[6], const double own[4], int f, gcn10_aggregate_geom *out)
{
    int x0 = 0, x1 = W, y0 = 0, y1 = H;

    memset(out, 0, sizeof *out);
    if (f < 2 || f > 256 || W <= 0 || H <= 0 || !(gt[1] > 0.0) || !(gt[5] < 0.0) || gt[2] != 0.0 || gt[4] != 0.0 ||
        !isfinite(gt[0]) || !isfinite(gt[3]) || !isfinite(gt[1]) || !isfinite(gt[5]))
        return -1;
    if (own)
        gcn10_owned_window(gt, W, H, own, &x0, &x1, &y0, &y1);
    if (x0 >= x1 || y0 >= y1)
        return -1;
    out->x0 = x0;
    out->x1 = x1;
    out->y0 = y0;
    out->y1 = y1;
    out->Wa = (x1 - x0 + f - 1) / f;
    out->Ha = (y1 - y0 + f - 1) / f;
    out->gt[0] = gt[0] + (double)x0 * gt[1];
    out->gt[1] = (double)f * gt[1];
    out->gt[2] = 0.0;
    out->gt[3] = gt[3] + (double)y0 * gt[5];
    out->gt[4] = 0.0;
    out->gt[5] = (double)f * gt[5];
    return 0;
}

int gcn10_aggregate_start(struct run *r)
{
    const char *why = NULL;

    if (r->zonal)
        why = "aggregate cannot be combined with --zonal";
    else if (r->verify)
        why = "aggregate cannot be combined with --verify (aggregated rasters are not verified)";
    if (why) {
        fprintf(stderr, "[rank 0] %s\n", why);
        return -1;
    }
    snprintf(r->out_suffix, sizeof r->out_suffix, "_x%d", r->aggregate);
    return 0;
}

/* the input side: the block's grid of cells, which is what its files hold */
static int aggregate_plan_block(struct worker *w, struct block_in *in, const double own[4])
{
    if (gcn10_aggregate_geometry(in->W, in->H, in->gt, own, w->run->aggregate, &in->agg) != 0) {
        wlog(w, "ERROR", true, "aggregate block %d: the %d x %d window owns no pixel of its block, or is not north up",
             in->block_id, in->W, in->H);
        return 1;
    }
    in->out_W = in->agg.Wa;
    in->out_H = in->agg.Ha;
    memcpy(in->out_gt, in->agg.gt, sizeof in->out_gt);
    return 0;
}

/* the block reduced into the worker's overview buffers and handed to the encoder and the sink as premade rasters */
static int aggregate_strips(struct worker *w, struct block_in *in, gcn10_tiff_writer *tifs[GCN10_N_RASTERS])
{
    struct run *r = w->run;
    const struct gcn10_gpu_api *g = r->gpu;
    const gcn10_aggregate_geom *a = &in->agg;
    const int f = r->aggregate;
    const size_t slot = ((size_t)a->Wa * (size_t)a->Ha + 255) & ~(size_t)255;
    const int n_strips = (a->Ha + w->strip_rows - 1) / w->strip_rows;
    const uint8_t **tab;

    wlog(w, "INFO", false, "aggregate block %d: %d x %d cells of %d x %d px", in->block_id, a->Wa, a->Ha, f, f);
    if (gcn10_ensure_dev_on(w, w->ctx, (void **)&w->d_ov, &w->ov_cap, slot * (size_t)r->n_sel) != 0 ||
        gcn10_ensure_dev_on(w, w->ctx, &w->d_ov_ptrs, &w->ov_ptrs_cap,
                            (size_t)n_strips * GCN10_N_RASTERS * sizeof(void *)) != 0)
        return -1;
    {
        /* one band: a block of at most 2^31 - 1 pixels never has more workgroups than a grid holds */
        uint8_t *outs[GCN10_N_RASTERS] = { 0 };

        for (int q = 0; q < r->n_sel; q++)
            outs[q] = w->d_ov + (size_t)q * slot;
        GPU_OR_RETURN(w, -1, g->aggregate(w->ctx, in->d_block + (size_t)a->y0 * (size_t)in->W, in->W, a->y1 - a->y0,
                                          in->d_cj + a->y0, a->x0, a->x1, f, r->cond_mask, r->table_mask, outs,
                                          (size_t)a->Wa, w->s_kernel));
    }
    /* the rasters as strips of the encoder: strip s's n_sel pointers at [s][GCN10_N_RASTERS] */
    tab = calloc((size_t)n_strips * GCN10_N_RASTERS, sizeof *tab);
    if (!tab) {
        wlog(w, "ERROR", true, "malloc failed for the strips of block %d", in->block_id);
        return -1;
    }
    for (int s = 0; s < n_strips; s++)
        for (int q = 0; q < r->n_sel; q++)
            tab[(size_t)s * GCN10_N_RASTERS + q] =
                w->d_ov + (size_t)q * slot + (size_t)s * (size_t)w->strip_rows * (size_t)a->Wa;
    if (g->memcpy_h2d(w->ctx, w->d_ov_ptrs, tab, (size_t)n_strips * GCN10_N_RASTERS * sizeof *tab, w->s_kernel) != 0 ||
        g->stream_sync(w->ctx, w->s_kernel) != 0) {
        wlog(w, "ERROR", true, "gpu: %s", g->last_error());
        free(tab);
        return -1;
    }
    free(tab);
    return gcn10_run_strips(w, a->Wa, a->Ha, NULL, NULL, (const uint8_t *const *)w->d_ov_ptrs, NULL, tifs);
}

static int aggregate_finish(struct run *r, gcn10_log *log0)
{
    char msg[256];
    int blocks = 0;

    for (int i = 0; i < r->n_workers; i++)
        blocks += r->workers[i].blocks_done;
    snprintf(msg, sizeof msg, "aggregate: %d blocks, %d rasters each, cells of %d x %d px, under cn_rasters_<cond>_x%d/",
             blocks, r->n_sel, r->aggregate, r->aggregate, r->aggregate);
    gcn10_log_message(log0, "INFO", msg, true);
    return 0;
}

/* the write path with premade rasters: a block that cannot be planned or read is given up as a write run gives it up */
const struct gcn10_mode gcn10_mode_aggregate = {
    .writes_block_files = true, .plan_block = aggregate_plan_block, .block = gcn10_encode_block, .strips = aggregate_strips,
    .finish = aggregate_finish,
};
