/* zonal.c -- composite curve numbers per zone (config key "zonal", --zonal / --zones): no counterpart in the reference.
 *
 * A zonal run writes no raster.  Every block is staged as for a write run (input thread, GPU inflate, prepare_tile);
 * the input side also scan-converts the zones over the block (zones.c), so that this overlaps the block before.  The
 * worker uploads the spans and items from pinned memory, runs gcn10_gpu_zonal_pair_histogram over the decoded
 * landcover block, and takes the local zones' pair histograms back -- in batches, so that device and pinned memory
 * stay bounded whatever the shapefile holds.  The host turns a zone's pair histogram into the selected rasters'
 * histograms (gcn10_raster_histogram) and adds pixels, valid pixels (value != 255, whatever "nodata" says: 255 is
 * never a curve number), sum, sum of squares, min and max into one table of the whole process.  All of it is
 * integers, so the table does not depend on the order in which the workers of all GPUs add to it.  With a design storm
 * (config key "storm", runoff.c) the sum of the storm's runoff table over the valid pixels is added up as well, from the
 * same histograms, and the table gets the columns runoff_mm,cn_runoff; with several storms (config key "storms") one
 * such sum and the columns runoff_mm_p<N>,cn_runoff_p<N> per storm.
 *
 * With a rainfall raster under the zones (config key "zone_rain", include/gcn10_host.h "A rainfall raster under the
 * zones") the depth differs from pixel to pixel of a zone, so no histogram of the zone gives its runoff.  The input side
 * also plans the block on the raster's grid and cuts the zones' spans where the raster's byte changes
 * (gcn10_zone_rain_cut); after the histogram pass, which is unchanged, the worker uploads the cut spans and items in
 * the same kind of batches, clears nz x n_sel triples, runs gcn10_gpu_zonal_sums_rain -- the reduction against the 256
 * tables happens on the device -- and takes the triples back: 24 bytes per (zone, raster).  The table adds them, and
 * the cutter's rain_pixels and rain_sum per zone, under its mutex: integers again.
 *
 * With several such rasters (config key "zone_rains", "Several rainfall rasters under the zones" there) the spans are cut
 * where the byte of ANY layer changes (gcn10_zone_rains_cut), the same batches run gcn10_gpu_zonal_sums_rains, and a
 * (zone, raster) brings back 2 + K words: s and n once, sw_j per layer.  "zone_rain" keeps its own cut and call.
 */
#include "pipeline_internal.h"

#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#define wlog gcn10_wlog

/* Zones and spans of one kernel call.  1024 zones are 32 MiB of pair histograms on the device and as much pinned
 * memory per worker, 2^20 spans another 16 MiB; a block with more is done in several calls (a zone may be cut between
 * two of them: everything the table keeps adds up).  The batch is sized by memory, not by time: a call over 1 000
 * zones takes 0.06 ms and one over 100 000 zones 0.5 ms (profiles/zonal/kernel_bounds.json, "small_zones"), 5 us per
 * 1 000 zones either way, so a larger batch would save microseconds per block.  What a block costs on the host is
 * not measured yet (DESIGN.md "Zonal composites"). */
enum { ZONE_BATCH = 1024, SPAN_BATCH = 1 << 20 };

struct zcell {
    uint64_t pixels, valid, sum, sum2;
    uint64_t runoff[GCN10_MAX_STORMS];      /* per storm, the sum of runoff_q[value] over the valid pixels */
    uint64_t rain[2 + GCN10_MAX_RAINS];     /* zone_rain / zone_rains: {s, n, sw_1 .. sw_K} over the valid pixels that lie
                                               in a rain cell */
    int min, max;
};

struct gcn10_zonal_table {
    pthread_mutex_t mu;
    struct zcell *cell;         /* [zones.n][n_sel] */
    uint64_t *rain_pixels, *rain_sum;       /* zone_rain / zone_rains: [zones.n] pixels in a rain cell, and [K][zones.n]
                                               the sum of every layer's bytes over them */
    int blocks;                 /* blocks counted */
};

struct gcn10_zonal_state {
    gcn10_zone_span *h_spans, *d_spans;     /* h_* pinned */
    gcn10_zone_item *h_items, *d_items;
    unsigned long long *h_hist, *d_hist;
    size_t h_spans_cap, d_spans_cap, h_items_cap, d_items_cap, h_hist_cap, d_hist_cap;
    struct zcell *part;                     /* [ZONE_BATCH][n_sel]: a batch, before it goes into the table */
    /* zone_rain: the cut spans, their items and the triples of a batch */
    gcn10_zone_span *h_rspans, *d_rspans;
    void *h_ritems, *d_ritems;              /* gcn10_zone_rain_item or gcn10_zone_rains_item: 16 bytes either way */
    unsigned long long *h_acc, *d_acc;
    size_t h_rspans_cap, d_rspans_cap, h_ritems_cap, d_ritems_cap, h_acc_cap, d_acc_cap;
    bool rain_tables_set;                   /* this worker's context holds the 256 tables */
};

int gcn10_zonal_start(struct run *r)
{
    char err[1024] = "";
    struct gcn10_zonal_table *t;

    if (gcn10_zones_open(r->cfg.zones_shp_path, r->cfg.zones_id_field, &r->zones, err, sizeof err) != 0) {
        fprintf(stderr, "[rank 0] %s\n", err);
        return -1;
    }
    t = calloc(1, sizeof *t);
    if (t)
        t->cell = calloc((size_t)(r->zones.n > 0 ? r->zones.n : 1) * (size_t)(r->n_sel > 0 ? r->n_sel : 1), sizeof *t->cell);
    if (t && t->cell && r->zone_rain_on) {
        t->rain_pixels = calloc((size_t)(r->zones.n > 0 ? r->zones.n : 1), sizeof *t->rain_pixels);
        t->rain_sum = calloc((size_t)(r->zones.n > 0 ? r->zones.n : 1) * (size_t)r->n_zone_rains, sizeof *t->rain_sum);
    }
    if (!t || !t->cell || (r->zone_rain_on && (!t->rain_pixels || !t->rain_sum))) {
        fprintf(stderr, "[rank 0] out of memory for the table of %d zones\n", r->zones.n);
        if (t) {
            free(t->cell);
            free(t->rain_pixels);
            free(t->rain_sum);
        }
        free(t);
        gcn10_zones_free(&r->zones);
        return -1;
    }
    for (size_t i = 0; i < (size_t)r->zones.n * (size_t)r->n_sel; i++) {
        t->cell[i].min = 255;
        t->cell[i].max = 0;
    }
    pthread_mutex_init(&t->mu, NULL);
    r->zonal_table = t;
    return 0;
}

static void zonal_teardown(struct worker *w)
{
    const struct gcn10_gpu_api *g = w->run->gpu;
    struct gcn10_zonal_state *z = w->zonal;

    if (!z)
        return;
    if (w->ctx) {
        if (z->h_spans) g->host_free(w->ctx, z->h_spans);
        if (z->h_items) g->host_free(w->ctx, z->h_items);
        if (z->h_hist) g->host_free(w->ctx, z->h_hist);
        if (z->d_spans) g->free(w->ctx, z->d_spans);
        if (z->d_items) g->free(w->ctx, z->d_items);
        if (z->d_hist) g->free(w->ctx, z->d_hist);
        if (z->h_rspans) g->host_free(w->ctx, z->h_rspans);
        if (z->h_ritems) g->host_free(w->ctx, z->h_ritems);
        if (z->h_acc) g->host_free(w->ctx, z->h_acc);
        if (z->d_rspans) g->free(w->ctx, z->d_rspans);
        if (z->d_ritems) g->free(w->ctx, z->d_ritems);
        if (z->d_acc) g->free(w->ctx, z->d_acc);
    }
    free(z->part);
    free(z);
    w->zonal = NULL;
}

static void zonal_block_unreadable(struct worker *w, int block_id)
{
    wlog(w, "ERROR", true, "zonal block %d: its landcover or soil window could not be read; the table lacks this block",
         block_id);
    atomic_store(&w->run->incomplete, 1);
}

/* the input side: the zones over the staged block, while the block before is counted */
static int zonal_plan_block(struct worker *w, struct block_in *in, const double own[4])
{
    struct run *r = w->run;
    char err[1024] = "";
    const double t0 = gcn10_now_seconds();

    gcn10_zone_plan_free(&in->zplan);
    if (gcn10_zones_build_plan(&r->zones, in->gt, in->W, in->H, own, 0, 0, &in->zplan, err, sizeof err) != 0) {
        wlog(w, "ERROR", true, "zonal block %d: %s", in->block_id, err);
        return -1;
    }
    if (r->zone_rain_on) {
        /* the block on the raster's grid -- ownership is in the spans already --, and the spans cut at its bytes */
        const gcn10_grid *zg = &r->zone_rain_grid;

        gcn10_grid_plan_free(&in->zr_gplan);
        gcn10_zone_rain_plan_free(&in->zr_cut);
        gcn10_zone_rains_plan_free(&in->zrs_cut);
        if (gcn10_grid_plan_block(zg, in->W, in->H, in->gt, NULL, &in->zr_gplan) != 0 ||
            (r->zone_rains_key
                 ? gcn10_zone_rains_cut(&in->zplan, in->W, in->H, in->zr_gplan.cellx, in->zr_gplan.celly, in->zr_gplan.cx0,
                                        in->zr_gplan.cy0, (const uint8_t *const *)r->zone_rain_layer, r->n_zone_rains,
                                        zg->nx, zg->ny, 0, 0, &in->zrs_cut)
                 : gcn10_zone_rain_cut(&in->zplan, in->W, in->H, in->zr_gplan.cellx, in->zr_gplan.celly, in->zr_gplan.cx0,
                                       in->zr_gplan.cy0, r->zone_rain_layer[0], zg->nx, zg->ny, 0, 0, &in->zr_cut)) != 0) {
            wlog(w, "ERROR", true, "zonal block %d: out of memory for the spans under the rainfall raster", in->block_id);
            return -1;
        }
    }
    w->t_zone_plan += gcn10_now_seconds() - t0;
    return 0;
}

/* one zone's pair histogram into the cells of the selected rasters: gcn10_raster_histogram, over the nonzero counters
 * only (a zone holds a few dozen of the 4096 pairs, and there are up to 18 rasters per zone) */
static void cells_of(const struct run *r, const uint64_t *pair, struct zcell *cell)
{
    uint16_t at[GCN10_PAIR_HIST_SIZE];
    uint64_t n[GCN10_PAIR_HIST_SIZE];
    size_t m = 0;

    for (int i = 0; i < GCN10_PAIR_HIST_SIZE; i++)
        if (pair[i]) {
            at[m] = (uint16_t)i;
            n[m++] = pair[i];
        }
    for (int q = 0; q < r->n_sel; q++) {
        const int k = r->sel[q];
        struct zcell *c = &cell[q];
        uint64_t hist[256];

        gcn10_raster_histogram_sparse(at, n, m, r->hist_codes, r->tables[k % 9], k / 9 == 0, hist);
        c->pixels = c->valid = c->sum = c->sum2 = 0;
        memset(c->runoff, 0, sizeof c->runoff);
        memset(c->rain, 0, sizeof c->rain);
        c->min = 255;
        c->max = 0;
        for (int v = 0; v < 256; v++) {
            if (!hist[v])
                continue;
            c->pixels += hist[v];
            if (v == GCN10_NODATA)
                continue;
            c->valid += hist[v];
            c->sum += hist[v] * (uint64_t)v;
            c->sum2 += hist[v] * (uint64_t)(v * v);
            for (int j = 0; r->storm_on && j < r->n_storms; j++)
                c->runoff[j] += hist[v] * (uint64_t)r->runoff_q[j][v];
            if (v < c->min)
                c->min = v;
            if (v > c->max)
                c->max = v;
        }
    }
}

/* first_span and n_spans of item i of either cut: both item structs begin with them */
static void item_spans(const void *items, size_t i, uint32_t *first_span, uint32_t *n_spans)
{
    uint32_t two[2];

    memcpy(two, (const char *)items + i * sizeof(gcn10_zone_rain_item), sizeof two);
    *first_span = two[0];
    *n_spans = two[1];
}

/* zone_rain / zone_rains: the words {s, n, sw_1 .. sw_K} of the block's local zones under the rainfall rasters, in batches
 * of at most ZONE_BATCH zones and SPAN_BATCH cut spans (one item at least); the table adds them.  0, or -1: a GPU call
 * failed (the caller logs it), or memory ran out (logged). */
static int zonal_rain_block(struct worker *w, struct block_in *in, bool *prepared)
{
    struct run *r = w->run;
    const struct gcn10_gpu_api *g = r->gpu;
    const bool many = r->zone_rains_key;
    const size_t n_items = many ? in->zrs_cut.n_items : in->zr_cut.n_items;
    const gcn10_zone_span *spans = many ? in->zrs_cut.spans : in->zr_cut.spans;
    const void *items = many ? (const void *)in->zrs_cut.items : (const void *)in->zr_cut.items;
    const gcn10_zone_plan *p = &in->zplan;
    struct gcn10_zonal_table *t = r->zonal_table;
    struct gcn10_zonal_state *z = w->zonal;
    const size_t item_size = sizeof(gcn10_zone_rain_item);
    const int words = many ? 2 + r->n_zone_rains : 3;
    const size_t row = (size_t)r->n_sel * (size_t)words;

    _Static_assert(sizeof(gcn10_zone_rain_item) == sizeof(gcn10_zone_rains_item), "one batch code for both item forms");
    if (n_items && !z->rain_tables_set) {
        if (g->set_rain_tables(w->ctx, r->zone_rain_q[0], 256) != 0)
            return -1;
        z->rain_tables_set = true;
    }
    for (size_t i0 = 0; i0 < n_items;) {
        uint32_t first_span, n_spans;
        size_t s0, i1 = i0, s1;
        int zone0, nz;

        item_spans(items, i0, &first_span, &n_spans);
        s0 = s1 = first_span;
        zone0 = spans[s0].zone;
        while (i1 < n_items) {
            item_spans(items, i1, &first_span, &n_spans);
            if (i1 > i0 && (spans[first_span].zone - zone0 >= ZONE_BATCH || first_span + n_spans - s0 > SPAN_BATCH))
                break;
            s1 = (size_t)first_span + n_spans;
            i1++;
        }
        nz = spans[s1 - 1].zone - zone0 + 1;

        if (gcn10_ensure_pinned_on(w, w->ctx, (void **)&z->h_rspans, &z->h_rspans_cap, (s1 - s0) * sizeof *z->h_rspans) != 0 ||
            gcn10_ensure_pinned_on(w, w->ctx, &z->h_ritems, &z->h_ritems_cap, (i1 - i0) * item_size) != 0 ||
            gcn10_ensure_pinned_on(w, w->ctx, (void **)&z->h_acc, &z->h_acc_cap, (size_t)nz * row * sizeof *z->h_acc) != 0 ||
            gcn10_ensure_dev_on(w, w->ctx, (void **)&z->d_rspans, &z->d_rspans_cap, (s1 - s0) * sizeof *z->d_rspans) != 0 ||
            gcn10_ensure_dev_on(w, w->ctx, &z->d_ritems, &z->d_ritems_cap, (i1 - i0) * item_size) != 0 ||
            gcn10_ensure_dev_on(w, w->ctx, (void **)&z->d_acc, &z->d_acc_cap, (size_t)nz * row * sizeof *z->d_acc) != 0)
            return -1;
        for (size_t s = s0; s < s1; s++) {
            z->h_rspans[s - s0] = spans[s];
            z->h_rspans[s - s0].zone -= zone0;
        }
        memcpy(z->h_ritems, (const char *)items + i0 * item_size, (i1 - i0) * item_size);
        for (size_t i = i0; i < i1; i++) {
            item_spans(items, i, &first_span, &n_spans);
            first_span -= (uint32_t)s0;
            memcpy((char *)z->h_ritems + (i - i0) * item_size, &first_span, sizeof first_span);
        }
        if (!*prepared) {
            if (g->prepare_tile(w->ctx, in->d_coarse, in->hsx, in->hsy, in->d_ci, in->W, w->s_kernel) != 0)
                return -1;
            *prepared = true;
        }
        if (g->memcpy_h2d(w->ctx, z->d_rspans, z->h_rspans, (s1 - s0) * sizeof *z->h_rspans, w->s_kernel) != 0 ||
            g->memcpy_h2d(w->ctx, z->d_ritems, z->h_ritems, (i1 - i0) * item_size, w->s_kernel) != 0 ||
            g->memset(w->ctx, z->d_acc, 0, (size_t)nz * row * sizeof *z->d_acc, w->s_kernel) != 0 ||
            (many ? g->zonal_sums_rains(w->ctx, in->d_block, in->W, in->H, in->d_cj, z->d_rspans, z->d_ritems, i1 - i0, nz,
                                        r->cond_mask, r->table_mask, r->n_zone_rains, z->d_acc, w->s_kernel)
                  : g->zonal_sums_rain(w->ctx, in->d_block, in->W, in->H, in->d_cj, z->d_rspans, z->d_ritems, i1 - i0, nz,
                                       r->cond_mask, r->table_mask, z->d_acc, w->s_kernel)) != 0 ||
            g->memcpy_d2h(w->ctx, z->h_acc, z->d_acc, (size_t)nz * row * sizeof *z->h_acc, w->s_kernel) != 0)
            return -1;
        {
            const double t0 = gcn10_now_seconds();

            if (g->stream_sync(w->ctx, w->s_kernel) != 0)
                return -1;
            w->t_gpu_wait += gcn10_now_seconds() - t0;
        }
        {
            const double t0 = gcn10_now_seconds();

            pthread_mutex_lock(&t->mu);
            for (int k = 0; k < nz; k++) {
                struct zcell *dst = &t->cell[(size_t)p->local_zone[zone0 + k] * (size_t)r->n_sel];
                const unsigned long long *src = z->h_acc + (size_t)k * row;

                for (int q = 0; q < r->n_sel; q++)
                    for (int word = 0; word < words; word++)
                        dst[q].rain[word] += src[words * q + word];
            }
            pthread_mutex_unlock(&t->mu);
            w->t_zone_accum += gcn10_now_seconds() - t0;
        }
        i0 = i1;
    }
    return 0;
}

static int zonal_block(struct worker *w, struct block_in *in)
{
    struct run *r = w->run;
    const struct gcn10_gpu_api *g = r->gpu;
    const gcn10_zone_plan *p = &in->zplan;
    struct gcn10_zonal_table *t = r->zonal_table;
    struct gcn10_zonal_state *z;
    const size_t row = (size_t)GCN10_PAIR_HIST_SIZE;
    bool prepared = false;

    if (!w->zonal) {
        w->zonal = calloc(1, sizeof *w->zonal);
        if (w->zonal)
            w->zonal->part = calloc((size_t)ZONE_BATCH * (size_t)(r->n_sel > 0 ? r->n_sel : 1), sizeof *w->zonal->part);
        if (!w->zonal || !w->zonal->part) {
            wlog(w, "ERROR", true, "out of memory for the zonal buffers");
            return -1;
        }
    }
    z = w->zonal;

    /* the block on the device, as for a write run */
    switch (gcn10_block_take(w, in)) {
    case GCN10_BLOCK_DEVICE_ERROR:
        goto gpu_fail;
    case GCN10_BLOCK_UNREADABLE:
        zonal_block_unreadable(w, in->block_id);
        return 0;
    }
    wlog(w, "INFO", false, "zonal block %d: %d zones, %zu spans", in->block_id, p->n_local, p->n_spans);

    /* batches of items: at most ZONE_BATCH zones and SPAN_BATCH spans each (one item at least) */
    for (size_t i0 = 0; i0 < p->n_items;) {
        const size_t s0 = p->items[i0].first_span;
        const int zone0 = p->spans[s0].zone;
        size_t i1 = i0, s1 = s0;
        int nz;

        while (i1 < p->n_items) {
            const gcn10_zone_item *it = &p->items[i1];

            if (i1 > i0 && (p->spans[it->first_span].zone - zone0 >= ZONE_BATCH ||
                            it->first_span + it->n_spans - s0 > SPAN_BATCH))
                break;
            s1 = (size_t)it->first_span + it->n_spans;
            i1++;
        }
        nz = p->spans[s1 - 1].zone - zone0 + 1;

        if (gcn10_ensure_pinned_on(w, w->ctx, (void **)&z->h_spans, &z->h_spans_cap, (s1 - s0) * sizeof *z->h_spans) != 0 ||
            gcn10_ensure_pinned_on(w, w->ctx, (void **)&z->h_items, &z->h_items_cap, (i1 - i0) * sizeof *z->h_items) != 0 ||
            gcn10_ensure_pinned_on(w, w->ctx, (void **)&z->h_hist, &z->h_hist_cap, (size_t)nz * row * sizeof *z->h_hist) != 0 ||
            gcn10_ensure_dev_on(w, w->ctx, (void **)&z->d_spans, &z->d_spans_cap, (s1 - s0) * sizeof *z->d_spans) != 0 ||
            gcn10_ensure_dev_on(w, w->ctx, (void **)&z->d_items, &z->d_items_cap, (i1 - i0) * sizeof *z->d_items) != 0 ||
            gcn10_ensure_dev_on(w, w->ctx, (void **)&z->d_hist, &z->d_hist_cap, (size_t)nz * row * sizeof *z->d_hist) != 0)
            return -1;
        for (size_t s = s0; s < s1; s++) {
            z->h_spans[s - s0] = p->spans[s];
            z->h_spans[s - s0].zone -= zone0;
        }
        for (size_t i = i0; i < i1; i++) {
            z->h_items[i - i0] = p->items[i];
            z->h_items[i - i0].first_span -= (uint32_t)s0;
        }
        if (!prepared) {
            if (g->prepare_tile(w->ctx, in->d_coarse, in->hsx, in->hsy, in->d_ci, in->W, w->s_kernel) != 0)
                goto gpu_fail;
            prepared = true;
        }
        if (g->memcpy_h2d(w->ctx, z->d_spans, z->h_spans, (s1 - s0) * sizeof *z->h_spans, w->s_kernel) != 0 ||
            g->memcpy_h2d(w->ctx, z->d_items, z->h_items, (i1 - i0) * sizeof *z->h_items, w->s_kernel) != 0 ||
            g->memset(w->ctx, z->d_hist, 0, (size_t)nz * row * sizeof *z->d_hist, w->s_kernel) != 0 ||
            g->zonal_pair_histogram(w->ctx, in->d_block, in->W, in->H, in->d_cj, z->d_spans, z->d_items, i1 - i0, nz,
                                    z->d_hist, w->s_kernel) != 0 ||
            g->memcpy_d2h(w->ctx, z->h_hist, z->d_hist, (size_t)nz * row * sizeof *z->h_hist, w->s_kernel) != 0)
            goto gpu_fail;
        {
            const double t0 = gcn10_now_seconds();

            if (g->stream_sync(w->ctx, w->s_kernel) != 0)
                goto gpu_fail;
            w->t_gpu_wait += gcn10_now_seconds() - t0;
        }
        {
            const double t0 = gcn10_now_seconds();

            for (int k = 0; k < nz; k++)
                cells_of(r, (const uint64_t *)z->h_hist + (size_t)k * row, &z->part[(size_t)k * (size_t)r->n_sel]);
            pthread_mutex_lock(&t->mu);
            for (int k = 0; k < nz; k++) {
                struct zcell *dst = &t->cell[(size_t)p->local_zone[zone0 + k] * (size_t)r->n_sel];
                const struct zcell *src = &z->part[(size_t)k * (size_t)r->n_sel];

                for (int q = 0; q < r->n_sel; q++) {
                    dst[q].pixels += src[q].pixels;
                    dst[q].valid += src[q].valid;
                    dst[q].sum += src[q].sum;
                    dst[q].sum2 += src[q].sum2;
                    for (int j = 0; j < GCN10_MAX_STORMS; j++)
                        dst[q].runoff[j] += src[q].runoff[j];
                    /* (the rain triples come from the pass of their own below) */
                    if (src[q].valid && src[q].min < dst[q].min)
                        dst[q].min = src[q].min;
                    if (src[q].valid && src[q].max > dst[q].max)
                        dst[q].max = src[q].max;
                }
            }
            pthread_mutex_unlock(&t->mu);
            w->t_zone_accum += gcn10_now_seconds() - t0;
        }
        i0 = i1;
    }
    if (r->zone_rain_on && zonal_rain_block(w, in, &prepared) != 0)
        goto gpu_fail;
    pthread_mutex_lock(&t->mu);
    for (int k = 0; r->zone_rain_on && !r->zone_rains_key && k < in->zr_cut.n_local; k++) {
        t->rain_pixels[p->local_zone[k]] += in->zr_cut.rain_pixels[k];
        t->rain_sum[p->local_zone[k]] += in->zr_cut.rain_sum[k];
    }
    for (int k = 0; r->zone_rains_key && k < in->zrs_cut.n_local; k++) {
        t->rain_pixels[p->local_zone[k]] += in->zrs_cut.rain_pixels[k];
        for (int j = 0; j < r->n_zone_rains; j++)
            t->rain_sum[(size_t)j * (size_t)r->zones.n + (size_t)p->local_zone[k]] += in->zrs_cut.rain_sum[j][k];
    }
    t->blocks++;
    pthread_mutex_unlock(&t->mu);
    return 0;

gpu_fail:
    wlog(w, "ERROR", true, "gpu: %s", g->last_error());
    if (w->ctx)
        g->stream_sync(w->ctx, w->s_kernel);
    return -1;
}

/* The table, through a temporary name and rename, and the closing console line.  The exit code: 0, or 1
 * when it could not be written. */
static int zonal_finish(struct run *r, gcn10_log *log0)
{
    struct gcn10_zonal_table *t = r->zonal_table;
    const char *path = r->cfg.zonal_output && *r->cfg.zonal_output ? r->cfg.zonal_output : "zonal_cn.csv";
    char tmp[PATH_MAX], msg[PATH_MAX + 256];
    int without = 0, rc = -1;
    FILE *f;

    snprintf(tmp, sizeof tmp, "%s.part.%ld", path, (long)getpid());
    f = fopen(tmp, "w");
    if (f) {
        const int n_storms = r->storm_on ? r->n_storms : 0;

        fprintf(f, "zone_id,condition,hc,arc,pixels,valid,sum,mean,min,max,stddev");
        for (int j = 0; j < n_storms; j++)      /* one storm: the plain names; several: the names carry N */
            if (n_storms == 1)
                fprintf(f, ",runoff_mm,cn_runoff");
            else
                fprintf(f, ",runoff_mm_p%u,cn_runoff_p%u", (unsigned)r->runoff_q[j][100], (unsigned)r->runoff_q[j][100]);
        if (r->zone_rain_on && r->n_zone_rains == 1)
            fprintf(f, ",rain_pixels,rain_mm,rain_valid,runoff_mm_rain,cn_runoff_rain");
        else if (r->zone_rain_on) {         /* several rasters: what is counted once, then three columns per raster */
            fprintf(f, ",rain_pixels,rain_valid");
            for (int j = 1; j <= r->n_zone_rains; j++)
                fprintf(f, ",rain_mm_rain%d,runoff_mm_rain%d,cn_runoff_rain%d", j, j, j);
        }
        fprintf(f, "\n");
        for (int i = 0; i < r->zones.n; i++) {
            if (r->n_sel > 0 && t->cell[(size_t)i * (size_t)r->n_sel].pixels == 0)
                without++;
            for (int q = 0; q < r->n_sel; q++) {
                const struct zcell *c = &t->cell[(size_t)i * (size_t)r->n_sel + (size_t)q];
                const int k = r->sel[q];

                fprintf(f, "%lld,%s,%s,%s,%llu,%llu,%llu,", (long long)r->zones.id[i], gcn10_conds[k / 9],
                        gcn10_hcs[(k % 9) / 3], gcn10_arcs[k % 3], (unsigned long long)c->pixels,
                        (unsigned long long)c->valid, (unsigned long long)c->sum);
                if (c->valid) {
                    /* the mean and the population standard deviation as gcn10_band_stats_of forms them */
                    const unsigned __int128 var = (unsigned __int128)c->sum2 * c->valid - (unsigned __int128)c->sum * c->sum;

                    fprintf(f, "%.14g,%d,%d,%.14g", (double)c->sum / (double)c->valid, c->min, c->max,
                            sqrt((double)var) / (double)c->valid);
                    for (int j = 0; j < n_storms; j++)  /* the zone's mean runoff depth, and the curve number that yields it */
                        fprintf(f, ",%.14g,%d", (double)c->runoff[j] / (double)c->valid / 100.0,
                                gcn10_runoff_cn(c->sum, c->valid, c->runoff[j], r->runoff_q[j]));
                }
                else {
                    fprintf(f, ",,,");
                    for (int j = 0; j < n_storms; j++)
                        fprintf(f, ",,");
                }
                if (r->zone_rain_on && r->n_zone_rains == 1) {  /* include/gcn10_host.h "A rainfall raster under the zones" */
                    double rain_mm, runoff_mm;
                    int cn;
                    const int have = gcn10_zone_rain_values(t->rain_pixels[i], t->rain_sum[i], r->zone_rain_unit,
                                                            r->zone_rain_lambda, c->rain[0], c->rain[1], c->rain[2],
                                                            &rain_mm, &runoff_mm, &cn);

                    fprintf(f, ",%llu,", (unsigned long long)t->rain_pixels[i]);
                    if (have & 1)
                        fprintf(f, "%.14g", rain_mm);
                    fprintf(f, ",%llu,", (unsigned long long)c->rain[1]);
                    if (have & 2)
                        fprintf(f, "%.14g,%d", runoff_mm, cn);
                    else
                        fprintf(f, ",");
                }
                else if (r->zone_rain_on) { /* ... "Several rainfall rasters under the zones" */
                    fprintf(f, ",%llu,%llu", (unsigned long long)t->rain_pixels[i], (unsigned long long)c->rain[1]);
                    for (int j = 0; j < r->n_zone_rains; j++) {
                        double rain_mm, runoff_mm;
                        int cn;
                        const int have = gcn10_zone_rain_values(t->rain_pixels[i],
                                                                t->rain_sum[(size_t)j * (size_t)r->zones.n + (size_t)i],
                                                                r->zone_rain_unit, r->zone_rain_lambda, c->rain[0], c->rain[1],
                                                                c->rain[2 + j], &rain_mm, &runoff_mm, &cn);

                        fprintf(f, ",");
                        if (have & 1)
                            fprintf(f, "%.14g", rain_mm);
                        if (have & 2)
                            fprintf(f, ",%.14g,%d", runoff_mm, cn);
                        else
                            fprintf(f, ",,");
                    }
                }
                fprintf(f, "\n");
            }
        }
        {
            const bool bad = fflush(f) != 0 || ferror(f);

            if (fclose(f) == 0 && !bad && rename(tmp, path) == 0)
                rc = 0;
            else
                unlink(tmp);
        }
    }
    if (rc != 0) {
        snprintf(msg, sizeof msg, "zonal: cannot write the table %s", path);
        gcn10_log_message(log0, "ERROR", msg, true);
        return 1;
    }
    snprintf(msg, sizeof msg, "zonal: %d blocks, %d zones, %d without pixels, table %s", t->blocks, r->zones.n, without, path);
    gcn10_log_message(log0, "INFO", msg, true);
    return 0;
}

static void zonal_end(struct run *r)
{
    if (r->zonal_table) {
        pthread_mutex_destroy(&r->zonal_table->mu);
        free(r->zonal_table->cell);
        free(r->zonal_table->rain_pixels);
        free(r->zonal_table->rain_sum);
        free(r->zonal_table);
        r->zonal_table = NULL;
    }
    gcn10_zones_free(&r->zones);
}

static void zonal_plan_free(struct block_in *in)
{
    gcn10_zone_plan_free(&in->zplan);
    gcn10_grid_plan_free(&in->zr_gplan);
    gcn10_zone_rain_plan_free(&in->zr_cut);
    gcn10_zone_rains_plan_free(&in->zrs_cut);
}

const struct gcn10_mode gcn10_mode_zonal = {
    .plan_block = zonal_plan_block, .plan_free = zonal_plan_free, .block = zonal_block,
    .block_unreadable = zonal_block_unreadable, .worker_teardown = zonal_teardown,
    .finish = zonal_finish, .end = zonal_end,
};
