/* runoff_raster.c -- the runoff_rain run (config key "runoff_rain", --runoff-rain): no counterpart in the reference.
 *
 * A write run whose strips hold, instead of the curve number of every pixel, its runoff depth under a rainfall raster:
 * runoff_rasters_<cond>/q_<hc>_<arc>_<id>.tif, one file per block and selected raster, laid out as the block's CN raster
 * is.  The raster IS a gcn10_grid (gcn10_rain_raster_load), read once before any GPU is opened; the run holds its counts,
 * the 256 runoff tables of its unit (gcn10_rain_tables) as bytes of the output unit (gcn10_runoff_bytes), and every
 * worker hands those to its context once (gcn10_gpu_set_cell_byte_tables).
 *
 * Per block, the input side lays the raster's grid over the window (gcn10_grid_plan_block without an ownership box:
 * every pixel of the window is written, as in the CN rasters); the worker sends the two maps and the counts of the block's
 * cell rectangle up behind the staged block and runs gcn10_run_strips with gcn10_gpu_runoff_strip in the place of
 * cn_strip; the per-raster encoder and the sink follow as in a write run.  A block that meets no rain cell goes the same
 * way with maps that name no cell, and its files are all 255.
 */
#include "pipeline_internal.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define wlog gcn10_wlog

struct gcn10_runoff_state {
    void *h_up, *d_up;          /* cellx[W], celly[H], then the counts of the cell rectangle; h_up pinned */
    size_t h_up_cap, d_up_cap;
    bool tables_set;            /* the context has the 256 byte tables */
};

int gcn10_runoff_start(struct run *r)
{
    const gcn10_run_options *opt = &r->opt;
    const char *why = NULL;
    char err[2048] = "";
    uint16_t (*q)[256];
    int factor = r->cfg.aggregate;

    if (opt->runoff_rain) {
        free(r->cfg.runoff_rain);
        r->cfg.runoff_rain = strdup(opt->runoff_rain);
    }
    if (opt->runoff_rain_unit) {
        free(r->cfg.runoff_rain_unit);
        r->cfg.runoff_rain_unit = strdup(opt->runoff_rain_unit);
    }
    if (opt->runoff_unit) {
        free(r->cfg.runoff_unit);
        r->cfg.runoff_unit = strdup(opt->runoff_unit);
    }
    r->runoff_on = r->cfg.runoff_rain != NULL;
    if (r->cfg.runoff_rain_unit && !r->runoff_on) {
        fprintf(stderr, "[rank 0] runoff_rain_unit needs runoff_rain\n");
        return -1;
    }
    if (r->cfg.runoff_unit && !r->runoff_on) {
        fprintf(stderr, "[rank 0] runoff_unit needs runoff_rain\n");
        return -1;
    }
    if (!r->runoff_on)
        return 0;

    /* the order of include/gcn10_host.h */
    if (opt->aggregate && gcn10_parse_aggregate(opt->aggregate, &factor) != 0)
        factor = 1;                         /* a bad value asks for an aggregate run all the same */
    if (r->verify)
        why = "--verify";
    else if (factor)
        why = "aggregate";
    else if (r->cfg.zonal || opt->zonal || opt->zones)
        why = "--zonal";
    else if (opt->grid || r->cfg.grid)
        why = "grid";
    else if (opt->storm || r->cfg.storm)
        why = "storm";
    else if (opt->storms || r->cfg.storms)
        why = "storms";
    else if (opt->rain || r->cfg.rain)
        why = "rain";
    else if (opt->rains || r->cfg.rains)
        why = "rains";
    else if (opt->zone_rain || r->cfg.zone_rain)
        why = "zone_rain";
    else if (opt->zone_rains || r->cfg.zone_rains)
        why = "zone_rains";
    else if (r->cfg.cog)
        why = "cog";
    else if (r->cfg.stats)
        why = "stats";
    if (why) {
        fprintf(stderr, "[rank 0] runoff_rain cannot be combined with %s\n", why);
        return -1;
    }
    r->runoff_rain_unit = 1.0;
    r->runoff_lambda = 0.2;
    if (r->cfg.runoff_rain_unit &&
        gcn10_parse_rain_unit(r->cfg.runoff_rain_unit, &r->runoff_rain_unit, &r->runoff_lambda) != 0) {
        fprintf(stderr, "[rank 0] bad value for runoff_rain_unit: '%s' (unit[,lambda]: 0 < unit, 255 unit <= 650 mm, 0 <= "
                        "lambda < 1)\n", r->cfg.runoff_rain_unit);
        return -1;
    }
    r->runoff_u = gcn10_runoff_unit_of(r->runoff_rain_unit);
    if (r->cfg.runoff_unit && gcn10_parse_runoff_unit(r->cfg.runoff_unit, &r->runoff_u) != 0) {
        fprintf(stderr, "[rank 0] bad value for runoff_unit: '%s' (millimetres per count, 0.01 to 650)\n",
                r->cfg.runoff_unit);
        return -1;
    }
    if (gcn10_rain_raster_load("runoff_rain", r->cfg.runoff_rain, &r->runoff_grid, &r->runoff_layer, err, sizeof err) != 0) {
        fprintf(stderr, "[rank 0] %s\n", err);
        return -1;
    }
    /* the 256 runoff tables and their bytes, once per run */
    q = malloc(256 * sizeof *q);
    r->runoff_t = malloc(256 * sizeof *r->runoff_t);
    if (!q || !r->runoff_t) {
        fprintf(stderr, "[rank 0] out of memory for the tables of the rainfall raster\n");
        free(q);
        return -1;                          /* (runoff_end frees the rest) */
    }
    gcn10_rain_tables(r->runoff_rain_unit, r->runoff_lambda, q);
    gcn10_runoff_bytes(q, r->runoff_u, r->runoff_t);
    free(q);
    r->out_dir = "runoff_rasters";
    r->out_name = "q";
    return 0;
}

static void runoff_end(struct run *r)
{
    free(r->runoff_layer);
    free(r->runoff_t);
    r->runoff_layer = NULL;
    r->runoff_t = NULL;
}

/* the input side: the raster's grid over the staged block, while the block before is written */
static int runoff_plan_block(struct worker *w, struct block_in *in, const double own[4])
{
    (void)own;                              /* no ownership box: every pixel of the window is written */
    gcn10_grid_plan_free(&in->rr_gplan);
    if (gcn10_grid_plan_block(&w->run->runoff_grid, in->W, in->H, in->gt, NULL, &in->rr_gplan) != 0) {
        wlog(w, "ERROR", true, "runoff_rain block %d: the %d x %d window is not north up, or out of memory", in->block_id,
             in->W, in->H);
        return -1;
    }
    return 0;
}

static void runoff_plan_free(struct block_in *in)
{
    gcn10_grid_plan_free(&in->rr_gplan);
}

static void runoff_teardown(struct worker *w)
{
    const struct gcn10_gpu_api *g = w->run->gpu;
    struct gcn10_runoff_state *s = w->runoffst;

    if (!s)
        return;
    if (w->ctx) {
        if (s->h_up) g->host_free(w->ctx, s->h_up);
        if (s->d_up) g->free(w->ctx, s->d_up);
    }
    free(s);
    w->runoffst = NULL;
}

/* the block's maps and the counts of its cell rectangle behind the staged block, then the strips */
static int runoff_strips(struct worker *w, struct block_in *in, gcn10_tiff_writer *tifs[GCN10_N_RASTERS])
{
    struct run *r = w->run;
    const struct gcn10_gpu_api *g = r->gpu;
    const gcn10_grid_plan *p = &in->rr_gplan;
    const bool none = p->cx1 == p->cx0 || p->cy1 == p->cy0 || !p->cellx || !p->celly;   /* the block meets no rain cell */
    const int ncx = none ? 1 : p->cx1 - p->cx0, ncy = none ? 1 : p->cy1 - p->cy0;
    const size_t maps = ((size_t)in->W + (size_t)in->H) * sizeof(int32_t);
    const size_t up = maps + (size_t)ncx * (size_t)ncy;
    struct gcn10_runoff_strip_args args;
    struct gcn10_runoff_state *s;
    int rc;

    if (!w->runoffst && !(w->runoffst = calloc(1, sizeof *w->runoffst))) {
        wlog(w, "ERROR", true, "out of memory for the buffers of the rainfall raster");
        return -1;
    }
    s = w->runoffst;
    if (gcn10_ensure_pinned_on(w, w->ctx, &s->h_up, &s->h_up_cap, up) != 0 ||
        gcn10_ensure_dev_on(w, w->ctx, &s->d_up, &s->d_up_cap, up) != 0)
        return -1;
    if (!s->tables_set) {                   /* once per context */
        GPU_OR_RETURN(w, -1, g->set_cell_byte_tables(w->ctx, r->runoff_t[0], 256));
        s->tables_set = true;
    }
    if (none) {
        memset(s->h_up, 0xff, maps);        /* -1: in no cell */
        ((uint8_t *)s->h_up)[maps] = 0;
    }
    else {
        memcpy(s->h_up, p->cellx, (size_t)in->W * sizeof(int32_t));
        memcpy((char *)s->h_up + (size_t)in->W * sizeof(int32_t), p->celly, (size_t)in->H * sizeof(int32_t));
        for (int cy = 0; cy < ncy; cy++)
            memcpy((uint8_t *)s->h_up + maps + (size_t)cy * (size_t)ncx,
                   r->runoff_layer + (size_t)(p->cy0 + cy) * (size_t)r->runoff_grid.nx + (size_t)p->cx0, (size_t)ncx);
    }
    wlog(w, "INFO", false, "runoff_rain block %d: rain cells [%d, %d) x [%d, %d)", in->block_id, none ? 0 : p->cx0,
         none ? 0 : p->cx1, none ? 0 : p->cy0, none ? 0 : p->cy1);
    GPU_OR_RETURN(w, -1, g->memcpy_h2d(w->ctx, s->d_up, s->h_up, up, w->s_kernel));
    args.d_cellx = s->d_up;
    args.d_celly = args.d_cellx + in->W;
    args.d_cells = (const uint8_t *)s->d_up + maps;
    args.ncx = ncx;
    args.ncy = ncy;
    w->runoff = &args;
    rc = gcn10_run_strips(w, in->W, in->H, in->d_block, in->d_cj, NULL, NULL, tifs);
    w->runoff = NULL;
    return rc;
}

const struct gcn10_mode gcn10_mode_runoff = {
    .writes_block_files = true, .plan_block = runoff_plan_block, .plan_free = runoff_plan_free,
    .block = gcn10_encode_block, .strips = runoff_strips, .worker_teardown = runoff_teardown, .end = runoff_end,
};
