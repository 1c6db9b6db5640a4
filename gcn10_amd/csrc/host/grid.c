/* grid.c -- mean-CN rasters on a model grid that spans blocks (config key "grid", --grid): no counterpart in the
 * reference.
 *
 * A grid run writes no 10 m raster.  The grid is the user's: an origin, a cell size and a cell count in the
 * landcover's CRS (gcn10_grid); which pixels a cell holds is a rule on pixel centres, stated in include/gcn10_host.h
 * and evaluated here exactly as stated, in plain IEEE double (this file is built with -ffp-contract=off): a cell
 * index is found by a division and corrected with the rule's own comparisons, as first_index of zones.c does.
 *
 * Every block is staged as for a write run (input thread, GPU inflate, prepare_tile); the input side also lays the
 * grid over the block (gcn10_grid_plan_block): the block's rectangle of cells, the local cell column and row of every
 * owned pixel column and row, and which cells are complete -- every centre they can hold is this block's -- or shared
 * with other blocks.  The worker runs gcn10_gpu_grid_sums once over the block's owned rows into pairs {sum, count} per
 * (raster, cell) on the device, gcn10_gpu_grid_finish turns them into bytes and packs the shared cells' pairs, and
 * both come back through pinned memory.  The bytes of complete cells go straight into the run's rasters; the pairs of
 * shared cells are added up in a table of the whole process whose size follows the number of shared cells, and become
 * bytes after the last block.  All of it is integers, so the rasters do not depend on the order in which the workers of
 * all GPUs get there.  The rasters are written by the I/O pool through the host tile encoder: at most 64 Mpx each.
 *
 * With a design storm (config key "storm", runoff.c) the sums are triples {sum, count, sum of q[value]}: the worker hands
 * the storm's runoff table to its context once (gcn10_gpu_set_weights) and runs the weighted pair of calls, which also
 * gives the runoff-equivalent byte of every cell (gcn10_runoff_cn); the shared cells carry triples, and every selected
 * raster is written twice, its mean as without a storm and cnq_<hc>_<arc>_p<N>.tif beside it.  With K storms (config
 * key "storms") the sums are 2 + K words, word 2 + k the sum of storm k's table: one set of tables per context
 * (gcn10_gpu_set_weight_tables), the _storms pair of calls, K runoff-equivalent bytes per cell, and one
 * cnq_<hc>_<arc>_p<N_k>.tif per storm beside the mean.
 *
 * With a rainfall raster (config key "rain") the storm differs from cell to cell: the run holds the raster's nx x ny
 * counts and the 256 runoff tables of gcn10_rain_tables, the worker hands the tables to its context once
 * (gcn10_gpu_set_rain_tables), uploads the counts of the block's cell rectangle beside the maps and runs the _rain pair
 * of calls; triples as with one storm, the shared cells finished with the table of the cell's own count, and
 * cnq_<hc>_<arc>_rain.tif beside every mean.  With K rainfall rasters (config key "rains") the run holds K such rasters
 * and still one set of tables; the K byte rectangles of a block go up behind the maps, the _rains pair of calls counts the
 * block once into 2 + K words, the shared cells are finished per layer with the table of the cell's byte in that layer
 * (gcn10_rains_cell), and cnq_<hc>_<arc>_rain<j>.tif per raster stands beside every mean (one raster: _rain.tif).
 */
#include "pipeline_internal.h"

#include <errno.h>
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#define wlog gcn10_wlog

#if defined(__GNUC__) && !defined(__clang__)
#define NO_CONTRACT __attribute__((optimize("fp-contract=off")))
#else
#define NO_CONTRACT
#pragma STDC FP_CONTRACT OFF
#endif

/* ---------------------------------------------------------------------------------------------------------------- */
/* geometry                                                                                                          */
/* ---------------------------------------------------------------------------------------------------------------- */

int gcn10_parse_grid(const char *text, gcn10_grid *out)
{
    double d[4];
    long n[2];
    const char *p = text;
    char *end;

    if (!text)
        return -1;
    for (int i = 0; i < 6; i++) {
        /* strtod and strtol skip leading white space and take hexadecimal, "inf" and "nan": a field starts with a
         * sign, a digit or a point, and the values are checked below */
        if (!(*p == '-' || *p == '+' || *p == '.' || (*p >= '0' && *p <= '9')))
            return -1;
        errno = 0;
        if (i < 4)
            d[i] = strtod(p, &end);
        else
            n[i - 4] = strtol(p, &end, 10);
        if (end == p || errno != 0 || *end != (i < 5 ? ',' : '\0'))
            return -1;
        p = end + 1;
    }
    if (!isfinite(d[0]) || !isfinite(d[1]) || !isfinite(d[2]) || !isfinite(d[3]) || !(d[2] > 0.0) || !(d[3] > 0.0) ||
        n[0] < 1 || n[1] < 1 || n[0] > GCN10_GRID_MAX_CELLS || n[1] > GCN10_GRID_MAX_CELLS ||
        (long long)n[0] * (long long)n[1] > GCN10_GRID_MAX_CELLS)
        return -1;
    out->xmin = d[0];
    out->ymax = d[1];
    out->dx = d[2];
    out->dy = d[3];
    out->nx = (int)n[0];
    out->ny = (int)n[1];
    return 0;
}

NO_CONTRACT static inline double edge_x(const gcn10_grid *g, int k)
{
    return g->xmin + (double)k * g->dx;
}

NO_CONTRACT static inline double edge_y(const gcn10_grid *g, int k)
{
    return g->ymax - (double)k * g->dy;
}

/* the k in [0, n) an estimate stands for; the comparisons of the callers decide from there */
static int start_at(double est, int n)
{
    return !(est > 0.0) ? 0 : (est >= (double)(n - 1) ? n - 1 : (int)est);
}

/* the cell column of a centre: ex(k) <= px < ex(k+1), or -1 */
NO_CONTRACT static int column_of(const gcn10_grid *g, double px)
{
    int k;

    if (!(px >= edge_x(g, 0)) || !(px < edge_x(g, g->nx)))
        return -1;
    k = start_at(floor((px - g->xmin) / g->dx), g->nx);
    while (k > 0 && px < edge_x(g, k))
        k--;
    while (k < g->nx - 1 && px >= edge_x(g, k + 1))
        k++;
    return k;
}

/* the cell row of a centre: ey(k+1) < py <= ey(k), or -1 */
NO_CONTRACT static int row_of(const gcn10_grid *g, double py)
{
    int k;

    if (!(py <= edge_y(g, 0)) || !(py > edge_y(g, g->ny)))
        return -1;
    k = start_at(floor((g->ymax - py) / g->dy), g->ny);
    while (k > 0 && py > edge_y(g, k))
        k--;
    while (k < g->ny - 1 && py <= edge_y(g, k + 1))
        k++;
    return k;
}

void gcn10_grid_plan_free(gcn10_grid_plan *p)
{
    free(p->cellx);
    free(p->celly);
    free(p->complete_x);
    free(p->complete_y);
    free(p->shared);
    memset(p, 0, sizeof *p);
}

NO_CONTRACT int gcn10_grid_plan_block(const gcn10_grid *g, int W, int H, const double gt[6], const double own[4],
                                      gcn10_grid_plan *out)
{
    int x0 = 0, x1 = W, y0 = 0, y1 = H;
    int cx0 = INT_MAX, cx1 = 0, cy0 = INT_MAX, cy1 = 0, ncx, ncy;
    size_t n = 0;

    memset(out, 0, sizeof *out);
    if (W <= 0 || H <= 0 || !(gt[1] > 0.0) || !(gt[5] < 0.0) || gt[2] != 0.0 || gt[4] != 0.0 || !isfinite(gt[0]) ||
        !isfinite(gt[3]) || !isfinite(gt[1]) || !isfinite(gt[5]) || g->nx < 1 || g->ny < 1 || !(g->dx > 0.0) ||
        !(g->dy > 0.0))
        return -1;
    if (own)
        gcn10_owned_window(gt, W, H, own, &x0, &x1, &y0, &y1);
    out->x0 = x0;
    out->x1 = x1;
    out->y0 = y0;
    out->y1 = y1;
    out->cellx = malloc((size_t)W * sizeof *out->cellx);
    out->celly = malloc((size_t)H * sizeof *out->celly);
    if (!out->cellx || !out->celly) {
        gcn10_grid_plan_free(out);
        return -1;
    }
    for (int x = 0; x < W; x++) {
        const int k = x >= x0 && x < x1 ? column_of(g, gt[0] + (x + 0.5) * gt[1]) : -1;

        out->cellx[x] = k;
        if (k >= 0 && k < cx0)
            cx0 = k;
        if (k >= cx1)
            cx1 = k + 1;
    }
    for (int y = 0; y < H; y++) {
        const int k = y >= y0 && y < y1 ? row_of(g, gt[3] + (y + 0.5) * gt[5]) : -1;

        out->celly[y] = k;
        if (k >= 0 && k < cy0)
            cy0 = k;
        if (k >= cy1)
            cy1 = k + 1;
    }
    if (cx0 >= cx1 || cy0 >= cy1) {         /* no owned pixel in the grid: the block costs nothing */
        const int keep[4] = { x0, x1, y0, y1 };

        gcn10_grid_plan_free(out);
        out->x0 = keep[0];
        out->x1 = keep[1];
        out->y0 = keep[2];
        out->y1 = keep[3];
        return 0;
    }
    for (int x = 0; x < W; x++)
        if (out->cellx[x] >= 0)
            out->cellx[x] -= cx0;
    for (int y = 0; y < H; y++)
        if (out->celly[y] >= 0)
            out->celly[y] -= cy0;
    out->cx0 = cx0;
    out->cx1 = cx1;
    out->cy0 = cy0;
    out->cy1 = cy1;
    ncx = cx1 - cx0;
    ncy = cy1 - cy0;
    out->complete_x = calloc((size_t)ncx, 1);
    out->complete_y = calloc((size_t)ncy, 1);
    if (!out->complete_x || !out->complete_y) {
        gcn10_grid_plan_free(out);
        return -1;
    }
    for (int k = 0; own && k < ncx; k++)
        out->complete_x[k] = own[0] <= edge_x(g, cx0 + k) && edge_x(g, cx0 + k + 1) <= own[2];
    for (int k = 0; own && k < ncy; k++)
        out->complete_y[k] = own[1] <= edge_y(g, cy0 + k + 1) && edge_y(g, cy0 + k) <= own[3];
    for (int pass = 0; pass < 2; pass++) {  /* count the shared cells, then list them */
        n = 0;
        for (int cy = 0; cy < ncy; cy++)
            for (int cx = 0; cx < ncx; cx++)
                if (!(out->complete_y[cy] && out->complete_x[cx])) {
                    if (pass)
                        out->shared[n] = (uint32_t)((size_t)cy * (size_t)ncx + (size_t)cx);
                    n++;
                }
        if (!pass && n > 0 && !(out->shared = malloc(n * sizeof *out->shared))) {
            gcn10_grid_plan_free(out);
            return -1;
        }
    }
    out->n_shared = n;
    return 0;
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* the rainfall raster                                                                                               */
/* ---------------------------------------------------------------------------------------------------------------- */

int gcn10_rain_load(const char *path, const gcn10_grid *g, uint8_t **out, char *err, size_t errcap)
{
    char why[1024] = "";
    gcn10_raster *ra = gcn10_raster_open(path, NULL, why, sizeof why);
    const double none[6] = { 0.0, 1.0, 0.0, 0.0, 0.0, 1.0 };       /* what the reader reports without georeferencing */
    double gt[6];
    uint8_t *bytes;
    int w, h;

    *out = NULL;
    if (!ra) {
        snprintf(err, errcap, "rain: cannot read '%s': %s", path, why);
        return GCN10_RAIN_E_READ;
    }
    gcn10_raster_info(ra, &w, &h, gt);
    if (w != g->nx || h != g->ny) {
        snprintf(err, errcap, "rain: '%s' has %d x %d pixels, the grid has %d x %d cells", path, w, h, g->nx, g->ny);
        gcn10_raster_close(ra);
        return GCN10_RAIN_E_SIZE;
    }
    if (memcmp(gt, none, sizeof none) != 0 &&
        !(gt[0] == g->xmin && gt[3] == g->ymax && gt[1] == g->dx && gt[5] == -g->dy && gt[2] == 0.0 && gt[4] == 0.0)) {
        snprintf(err, errcap, "rain: '%s' does not lie on the grid (origin %.17g, %.17g, pixel %.17g x %.17g)", path,
                 gt[0], gt[3], gt[1], gt[5]);
        gcn10_raster_close(ra);
        return GCN10_RAIN_E_GEOTRANSFORM;
    }
    bytes = malloc((size_t)w * (size_t)h);
    if (!bytes || gcn10_raster_read(ra, 0, 0, w, h, bytes, why, sizeof why) != 0) {
        snprintf(err, errcap, "rain: cannot read '%s': %s", path, bytes ? why : "out of memory");
        free(bytes);
        gcn10_raster_close(ra);
        return GCN10_RAIN_E_READ;
    }
    gcn10_raster_close(ra);
    *out = bytes;
    return 0;
}

int gcn10_rains_load(const char *const files[], int k, const gcn10_grid *g, uint8_t *out[GCN10_MAX_RAINS], char *err,
                     size_t errcap)
{
    char why[PATH_MAX + 1200] = "";

    for (int j = 0; j < GCN10_MAX_RAINS; j++)
        out[j] = NULL;
    for (int j = 0; j < k; j++) {
        const int rc = gcn10_rain_load(files[j], g, &out[j], why, sizeof why);

        if (rc != 0) {
            for (int i = 0; i < j; i++) {
                free(out[i]);
                out[i] = NULL;
            }
            snprintf(err, errcap, "rains%s", why + strlen("rain"));     /* "rain: ..." as "rains: ..." */
            return rc;
        }
    }
    return 0;
}

int gcn10_rain_raster_load(const char *prefix, const char *path, gcn10_grid *grid, uint8_t **out, char *err,
                           size_t errcap)
{
    char why[1024] = "";
    gcn10_raster *ra = gcn10_raster_open(path, NULL, why, sizeof why);
    const double none[6] = { 0.0, 1.0, 0.0, 0.0, 0.0, 1.0 };       /* what the reader reports without georeferencing */
    double gt[6];
    uint8_t *bytes;
    int w, h;

    *out = NULL;
    memset(grid, 0, sizeof *grid);
    if (!ra) {
        snprintf(err, errcap, "%s: cannot read '%s': %s", prefix, path, why);
        return -1;
    }
    gcn10_raster_info(ra, &w, &h, gt);
    if (memcmp(gt, none, sizeof none) == 0)
        snprintf(err, errcap, "%s: '%s' carries no geotransform", prefix, path);
    else if (!(gt[1] > 0.0) || !(gt[5] < 0.0) || gt[2] != 0.0 || gt[4] != 0.0 || !isfinite(gt[0]) || !isfinite(gt[3]) ||
             !isfinite(gt[1]) || !isfinite(gt[5]))
        snprintf(err, errcap, "%s: '%s' is rotated or not north up", prefix, path);
    else if (w < 1 || h < 1 || (uint64_t)w * (uint64_t)h > (uint64_t)GCN10_GRID_MAX_CELLS)
        snprintf(err, errcap, "%s: '%s' has more than %d pixels", prefix, path, GCN10_GRID_MAX_CELLS);
    else {
        bytes = malloc((size_t)w * (size_t)h);
        if (!bytes || gcn10_raster_read(ra, 0, 0, w, h, bytes, why, sizeof why) != 0) {
            snprintf(err, errcap, "%s: cannot read '%s': %s", prefix, path, bytes ? why : "out of memory");
            free(bytes);
        }
        else {
            *grid = (gcn10_grid){ gt[0], gt[3], gt[1], -gt[5], w, h };
            *out = bytes;
        }
    }
    gcn10_raster_close(ra);
    return *out ? 0 : -1;
}

int gcn10_zone_rain_load(const char *path, gcn10_grid *grid, uint8_t **out, char *err, size_t errcap)
{
    return gcn10_rain_raster_load("zone_rain", path, grid, out, err, errcap);
}

int gcn10_zone_rains_load(const char *const files[], int k, gcn10_grid *grid, uint8_t *out[GCN10_MAX_RAINS], char *err,
                          size_t errcap)
{
    char why[1024 + PATH_MAX] = "";
    int rc = 0;

    for (int j = 0; j < GCN10_MAX_RAINS; j++)
        out[j] = NULL;
    memset(grid, 0, sizeof *grid);
    for (int j = 0; rc == 0 && j < k; j++) {
        gcn10_grid g;

        if (gcn10_zone_rain_load(files[j], j == 0 ? grid : &g, &out[j], why, sizeof why) != 0) {
            snprintf(err, errcap, "zone_rains%s", why + strlen("zone_rain"));   /* "zone_rain: ..." as "zone_rains: ..." */
            rc = -1;
        }
        else if (j > 0 && (g.nx != grid->nx || g.ny != grid->ny)) {
            snprintf(err, errcap, "zone_rains: '%s' has %d x %d pixels, '%s' has %d x %d", files[j], g.nx, g.ny, files[0],
                     grid->nx, grid->ny);
            rc = -1;
        }
        else if (j > 0 && (memcmp(&g.xmin, &grid->xmin, sizeof g.xmin) != 0 || memcmp(&g.ymax, &grid->ymax, sizeof g.ymax) != 0 ||
                           memcmp(&g.dx, &grid->dx, sizeof g.dx) != 0 || memcmp(&g.dy, &grid->dy, sizeof g.dy) != 0)) {
            snprintf(err, errcap, "zone_rains: '%s' does not lie on the grid of '%s' (origin %.17g, %.17g, pixel %.17g x %.17g)",
                     files[j], files[0], g.xmin, g.ymax, g.dx, -g.dy);     /* its gt[0], gt[3], gt[1], gt[5], as "rain" */
            rc = -1;
        }
    }
    if (rc != 0) {
        for (int j = 0; j < GCN10_MAX_RAINS; j++) {
            free(out[j]);
            out[j] = NULL;
        }
        memset(grid, 0, sizeof *grid);
    }
    return rc;
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* the run                                                                                                           */
/* ---------------------------------------------------------------------------------------------------------------- */

/* The rasters of the run, preset to 255, and the sums of the cells more than one block may add to: an open-addressed
 * table keyed by the cell's index in the grid, grown by doubling, so its size follows the number of shared cells. */
struct gcn10_grid_result {
    pthread_mutex_t mu;
    uint8_t *raster;            /* [n_sel][ny][nx] */
    uint8_t *cnq;               /* [n_cnq][n_sel][ny][nx], runoff-equivalent (storm and rain only) */
    uint32_t *key;              /* [cap]; NO_KEY: free */
    uint64_t *pair;             /* [cap][n_sel][words] = {s, n} or, with storms, {s, n, sw of every storm} */
    size_t cap, used;
    int n_sel, words;
    int n_cnq;                  /* runoff-equivalent rasters per selected raster: one per storm, one with rain */
    int blocks;                 /* blocks summed */
    gcn10_raster *esa;          /* the landcover, for its pixel size and its geo tags */
};
#define NO_KEY 0xffffffffu

struct gcn10_grid_state {
    void *h_up, *d_up;                      /* cellx | celly | shared indices; h_* pinned */
    unsigned long long *d_acc, *d_shared, *h_shared;
    uint8_t *d_means, *h_means;             /* the means, and with a storm the runoff-equivalent bytes behind them */
    size_t h_up_cap, d_up_cap, d_acc_cap, d_shared_cap, h_shared_cap, d_means_cap, h_means_cap;
    bool weights_set;                       /* the context has the storm's runoff table, or the 256 of the rain */
};

static size_t slot_of(const struct gcn10_grid_result *t, uint32_t key)
{
    size_t i = ((size_t)key * 2654435761u) & (t->cap - 1);

    while (t->key[i] != NO_KEY && t->key[i] != key)
        i = (i + 1) & (t->cap - 1);
    return i;
}

/* room for `more` further keys at a load of at most one half; 0 or -1 */
static int table_reserve(struct gcn10_grid_result *t, size_t more)
{
    size_t cap = t->cap ? t->cap : 1024;
    const size_t width = (size_t)t->n_sel * (size_t)t->words;
    uint32_t *okey = t->key;
    uint64_t *opair = t->pair;
    const size_t ocap = t->cap;

    while ((t->used + more) * 2 > cap)
        cap *= 2;
    if (cap == t->cap)
        return 0;
    t->key = malloc(cap * sizeof *t->key);
    t->pair = calloc(cap * width, sizeof *t->pair);
    if (!t->key || !t->pair) {
        free(t->key);
        free(t->pair);
        t->key = okey;
        t->pair = opair;
        return -1;
    }
    memset(t->key, 0xff, cap * sizeof *t->key);
    t->cap = cap;
    for (size_t i = 0; i < ocap; i++)
        if (okey[i] != NO_KEY) {
            const size_t at = slot_of(t, okey[i]);

            t->key[at] = okey[i];
            memcpy(t->pair + at * width, opair + i * width, width * sizeof *t->pair);
        }
    free(okey);
    free(opair);
    return 0;
}

static uint8_t mean_of(uint64_t s, uint64_t n)
{
    return n == 0 ? (uint8_t)GCN10_NODATA : (uint8_t)((2 * s + n) / (2 * n));
}

static void grid_end(struct run *r)
{
    struct gcn10_grid_result *t = r->grid_result;

    if (!t)
        return;
    gcn10_raster_close(t->esa);
    pthread_mutex_destroy(&t->mu);
    free(t->raster);
    free(t->cnq);
    free(t->key);
    free(t->pair);
    free(t);
    for (int j = 0; j < GCN10_MAX_RAINS; j++) {
        free(r->rain_layer[j]);
        r->rain_layer[j] = NULL;
    }
    free(r->rain_q);
    r->rain_q = NULL;
    r->grid_result = NULL;
}

int gcn10_grid_start(struct run *r)
{
    const gcn10_run_options *opt = &r->opt;
    const char *why = NULL;
    struct gcn10_grid_result *t;
    char err[PATH_MAX + 1200] = "";
    size_t bytes;

    if (gcn10_parse_grid(r->cfg.grid, &r->grid) != 0) {
        fprintf(stderr, "[rank 0] bad value for grid: '%s' (xmin,ymax,dx,dy,nx,ny)\n", r->cfg.grid);
        return -1;
    }
    gcn10_outer_from_env(&r->outer_rank, &r->outer_size);
    if (r->zonal)
        why = "grid cannot be combined with --zonal";
    else if (r->verify)
        why = "grid cannot be combined with --verify (the grid rasters are not verified)";
    else if (r->aggregate)
        why = "grid cannot be combined with aggregate";
    else if (opt->overwrite)
        why = "grid writes one raster per lookup and condition and cannot be combined with --overwrite";
    else if (r->outer_size > 1)
        why = "grid runs as one process: merging rasters across launcher ranks is not supported";
    else if (r->cfg.compress == GCN10_COMPRESS_LZW)
        why = "bad value for compress: 'lzw' with grid (the grid rasters are encoded on the host; there is no host LZW "
              "encoder)";
    if (why) {
        fprintf(stderr, "[rank 0] %s\n", why);
        return -1;
    }
    t = calloc(1, sizeof *t);
    if (!t) {
        fprintf(stderr, "[rank 0] out of memory for the grid rasters\n");
        return -1;
    }
    r->grid_result = t;
    pthread_mutex_init(&t->mu, NULL);
    t->n_sel = r->n_sel > 0 ? r->n_sel : 1;
    t->n_cnq = r->storm_on ? r->n_storms : (r->rain_on ? r->n_rains : 0);
    t->words = 2 + t->n_cnq;
    if (r->rain_on) {           /* the rasters on this grid, and the table of every count */
        if ((r->rains_key ? gcn10_rains_load(r->rain_file, r->n_rains, &r->grid, r->rain_layer, err, sizeof err)
                          : gcn10_rain_load(r->cfg.rain, &r->grid, &r->rain_layer[0], err, sizeof err)) != 0) {
            fprintf(stderr, "[rank 0] %s\n", err);
            grid_end(r);
            return -1;
        }
        r->rain_q = malloc(256 * sizeof *r->rain_q);
        if (!r->rain_q) {
            fprintf(stderr, "[rank 0] out of memory for the tables of the rainfall raster\n");
            grid_end(r);
            return -1;
        }
        gcn10_rain_tables(r->rain_unit, r->rain_lambda, r->rain_q);
    }
    /* the landcover's pixel size: below 8 pixels per cell the 10 m raster is the product (and a 16-pixel column group
     * of the kernel would meet more than three cell columns).  A landcover that does not open is the workers' to
     * report, block by block, as in every run. */
    t->esa = gcn10_raster_open(r->cfg.esa_data_path, r->cfg.esa_tile_dir, err, sizeof err);
    if (t->esa) {
        int rx, ry;
        double gt[6];

        gcn10_raster_info(t->esa, &rx, &ry, gt);
        if (r->grid.dx < 8.0 * fabs(gt[1]) || r->grid.dy < 8.0 * fabs(gt[5])) {
            fprintf(stderr, "[rank 0] bad value for grid: '%s' (cells under 8 landcover pixels of %.17g x %.17g)\n",
                    r->cfg.grid, fabs(gt[1]), fabs(gt[5]));
            grid_end(r);
            return -1;
        }
    }
    bytes = (size_t)t->n_sel * (size_t)r->grid.nx * (size_t)r->grid.ny;
    t->raster = malloc(bytes);
    if (t->n_cnq)
        t->cnq = malloc((size_t)t->n_cnq * bytes);
    if (!t->raster || (t->n_cnq && !t->cnq) || table_reserve(t, 0) != 0) {
        fprintf(stderr, "[rank 0] out of memory for the grid rasters (%zu bytes)\n", (size_t)(1 + t->n_cnq) * bytes);
        grid_end(r);
        return -1;
    }
    memset(t->raster, GCN10_NODATA, bytes);
    if (t->cnq)
        memset(t->cnq, GCN10_NODATA, (size_t)t->n_cnq * bytes);
    return 0;
}

static void grid_teardown(struct worker *w)
{
    const struct gcn10_gpu_api *g = w->run->gpu;
    struct gcn10_grid_state *s = w->gridst;

    if (!s)
        return;
    if (w->ctx) {
        if (s->h_up) g->host_free(w->ctx, s->h_up);
        if (s->h_shared) g->host_free(w->ctx, s->h_shared);
        if (s->h_means) g->host_free(w->ctx, s->h_means);
        if (s->d_up) g->free(w->ctx, s->d_up);
        if (s->d_acc) g->free(w->ctx, s->d_acc);
        if (s->d_shared) g->free(w->ctx, s->d_shared);
        if (s->d_means) g->free(w->ctx, s->d_means);
    }
    free(s);
    w->gridst = NULL;
}

static void grid_block_unreadable(struct worker *w, int block_id)
{
    wlog(w, "ERROR", true, "grid block %d: its landcover or soil window could not be read; the rasters lack this block",
         block_id);
    atomic_store(&w->run->incomplete, 1);
}

/* the input side: the grid over the staged block, while the block before is summed */
static int grid_plan_input(struct worker *w, struct block_in *in, const double own[4])
{
    gcn10_grid_plan_free(&in->gplan);
    if (gcn10_grid_plan_block(&w->run->grid, in->W, in->H, in->gt, own, &in->gplan) != 0) {
        wlog(w, "ERROR", true, "grid block %d: the %d x %d window is not north up, or out of memory", in->block_id,
             in->W, in->H);
        return -1;
    }
    return 0;
}

/* the block's bytes (cnq: the runoff-equivalent ones of every storm, NULL without a storm) and its shared cells' words
 * into the result of the run */
static int merge_block(struct run *r, const gcn10_grid_plan *p, const uint8_t *means, const uint8_t *cnq,
                       const uint64_t *shared)
{
    struct gcn10_grid_result *t = r->grid_result;
    const int ncx = p->cx1 - p->cx0, ncy = p->cy1 - p->cy0, nx = r->grid.nx;
    const size_t n_cells = (size_t)ncx * (size_t)ncy, plane = (size_t)nx * (size_t)r->grid.ny;
    const size_t words = (size_t)t->words, width = (size_t)t->n_sel * words;
    int a = 0, b;
    int rc = 0;

    /* the complete columns are consecutive (the edges never decrease): [a, b) */
    while (a < ncx && !p->complete_x[a])
        a++;
    for (b = a; b < ncx && p->complete_x[b]; b++)
        ;
    pthread_mutex_lock(&t->mu);
    for (int q = 0; q < t->n_sel && b > a; q++)
        for (int cy = 0; cy < ncy; cy++)
            if (p->complete_y[cy]) {
                const size_t to = (size_t)q * plane + (size_t)(p->cy0 + cy) * (size_t)nx + (size_t)(p->cx0 + a);
                const size_t from = (size_t)q * n_cells + (size_t)cy * (size_t)ncx + (size_t)a;

                memcpy(t->raster + to, means + from, (size_t)(b - a));
                for (size_t k = 0; cnq && k < words - 2; k++)
                    memcpy(t->cnq + k * (size_t)t->n_sel * plane + to, cnq + k * (size_t)t->n_sel * n_cells + from,
                           (size_t)(b - a));
            }
    if (table_reserve(t, p->n_shared) != 0)
        rc = -1;
    for (size_t i = 0; rc == 0 && i < p->n_shared; i++) {
        const uint32_t lc = p->shared[i];
        const uint32_t key = (uint32_t)((size_t)(p->cy0 + (int)(lc / (uint32_t)ncx)) * (size_t)nx +
                                        (size_t)(p->cx0 + (int)(lc % (uint32_t)ncx)));
        const size_t at = slot_of(t, key);

        if (t->key[at] == NO_KEY) {
            t->key[at] = key;
            t->used++;
        }
        for (int q = 0; q < t->n_sel; q++)
            for (size_t k = 0; k < words; k++)
                t->pair[at * width + words * (size_t)q + k] += shared[words * ((size_t)q * p->n_shared + i) + k];
    }
    if (rc == 0)
        t->blocks++;
    pthread_mutex_unlock(&t->mu);
    return rc;
}

static int grid_block(struct worker *w, struct block_in *in)
{
    struct run *r = w->run;
    const struct gcn10_gpu_api *g = r->gpu;
    const gcn10_grid_plan *p = &in->gplan;
    const int ncx = p->cx1 - p->cx0, ncy = p->cy1 - p->cy0;
    const size_t n_cells = (size_t)ncx * (size_t)ncy, n_sel = (size_t)r->n_sel;
    const size_t maps = ((size_t)in->W + (size_t)in->H) * sizeof(int32_t);
    const bool storm = r->storm_on, ladder = r->storms_key, rain = r->rain_on, layers = r->rains_key;
    const size_t n_storms = storm ? (size_t)r->n_storms : (rain ? (size_t)r->n_rains : 0);
    /* behind the maps and the shared indices, with rain: the counts of the block's cell rectangle, raster by raster */
    const size_t up = maps + p->n_shared * sizeof(uint32_t) + (rain ? n_storms * n_cells : 0);
    const size_t words = 2 + n_storms, bytes = (1 + n_storms) * n_sel * n_cells;    /* per cell: sums, and bytes back */
    struct gcn10_grid_state *s;
    int32_t *d_cellx, *d_celly;
    uint32_t *d_idx;
    uint8_t *d_rain;

    if (!w->gridst && !(w->gridst = calloc(1, sizeof *w->gridst))) {
        wlog(w, "ERROR", true, "out of memory for the grid buffers");
        return -1;
    }
    s = w->gridst;

    /* the block on the device, as for a write run */
    switch (gcn10_block_take(w, in)) {
    case GCN10_BLOCK_DEVICE_ERROR:
        goto gpu_fail;
    case GCN10_BLOCK_UNREADABLE:
        grid_block_unreadable(w, in->block_id);
        return 0;
    }
    wlog(w, "INFO", false, "grid block %d: cells [%d, %d) x [%d, %d), %zu shared with other blocks", in->block_id,
         p->cx0, p->cx1, p->cy0, p->cy1, p->n_shared);
    if (n_cells == 0) {                     /* the grid misses the block's owned pixels */
        pthread_mutex_lock(&r->grid_result->mu);
        r->grid_result->blocks++;
        pthread_mutex_unlock(&r->grid_result->mu);
        return 0;
    }
    if (gcn10_ensure_pinned_on(w, w->ctx, &s->h_up, &s->h_up_cap, up) != 0 ||
        gcn10_ensure_pinned_on(w, w->ctx, (void **)&s->h_means, &s->h_means_cap, bytes) != 0 ||
        gcn10_ensure_pinned_on(w, w->ctx, (void **)&s->h_shared, &s->h_shared_cap,
                               (n_sel * p->n_shared + 1) * words * sizeof *s->h_shared) != 0 ||
        gcn10_ensure_dev_on(w, w->ctx, &s->d_up, &s->d_up_cap, up) != 0 ||
        gcn10_ensure_dev_on(w, w->ctx, (void **)&s->d_acc, &s->d_acc_cap, n_sel * n_cells * words * sizeof *s->d_acc) != 0 ||
        gcn10_ensure_dev_on(w, w->ctx, (void **)&s->d_means, &s->d_means_cap, bytes) != 0 ||
        gcn10_ensure_dev_on(w, w->ctx, (void **)&s->d_shared, &s->d_shared_cap,
                            (n_sel * p->n_shared + 1) * words * sizeof *s->d_shared) != 0)
        return -1;
    if (storm && !s->weights_set) {         /* once per context: the tables are set before the first block */
        if ((ladder ? g->set_weight_tables(w->ctx, r->runoff_q[0], r->n_storms)
                    : g->set_weights(w->ctx, r->runoff_q[0])) != 0)
            goto gpu_fail;
        s->weights_set = true;
    }
    if (rain && !s->weights_set) {
        if (g->set_rain_tables(w->ctx, r->rain_q[0], 256) != 0)
            goto gpu_fail;
        s->weights_set = true;
    }
    memcpy(s->h_up, p->cellx, (size_t)in->W * sizeof(int32_t));
    memcpy((char *)s->h_up + (size_t)in->W * sizeof(int32_t), p->celly, (size_t)in->H * sizeof(int32_t));
    if (p->n_shared)
        memcpy((char *)s->h_up + maps, p->shared, p->n_shared * sizeof(uint32_t));
    d_cellx = s->d_up;
    d_celly = d_cellx + in->W;
    d_idx = (uint32_t *)((char *)s->d_up + maps);
    d_rain = (uint8_t *)s->d_up + maps + p->n_shared * sizeof(uint32_t);
    for (size_t j = 0; rain && j < n_storms; j++)
        for (int cy = 0; cy < ncy; cy++)
            memcpy((uint8_t *)s->h_up + maps + p->n_shared * sizeof(uint32_t) + j * n_cells + (size_t)cy * (size_t)ncx,
                   r->rain_layer[j] + (size_t)(p->cy0 + cy) * (size_t)r->grid.nx + (size_t)p->cx0, (size_t)ncx);
    if (g->memcpy_h2d(w->ctx, s->d_up, s->h_up, up, w->s_kernel) != 0 ||
        g->memset(w->ctx, s->d_acc, 0, n_sel * n_cells * words * sizeof *s->d_acc, w->s_kernel) != 0 ||
        g->prepare_tile(w->ctx, in->d_coarse, in->hsx, in->hsy, in->d_ci, in->W, w->s_kernel) != 0 ||
        (layers ? g->grid_sums_rains(w->ctx, in->d_block + (size_t)p->y0 * (size_t)in->W, in->W, p->y1 - p->y0,
                                     in->d_cj + p->y0, d_cellx, d_celly + p->y0, ncx, ncy, r->cond_mask, r->table_mask,
                                     d_rain, r->n_rains, s->d_acc, w->s_kernel) :
         rain ? g->grid_sums_rain(w->ctx, in->d_block + (size_t)p->y0 * (size_t)in->W, in->W, p->y1 - p->y0,
                                  in->d_cj + p->y0, d_cellx, d_celly + p->y0, ncx, ncy, r->cond_mask, r->table_mask,
                                  d_rain, s->d_acc, w->s_kernel)
              : (ladder ? g->grid_sums_storms : storm ? g->grid_sums_weighted : g->grid_sums)(
                    w->ctx, in->d_block + (size_t)p->y0 * (size_t)in->W, in->W, p->y1 - p->y0, in->d_cj + p->y0, d_cellx,
                    d_celly + p->y0, ncx, ncy, r->cond_mask, r->table_mask, s->d_acc, w->s_kernel)) != 0 ||
        (layers ? g->grid_finish_rains(w->ctx, s->d_acc, r->n_sel, n_cells, d_rain, r->n_rains, s->d_means,
                                       s->d_means + n_sel * n_cells, p->n_shared ? d_idx : NULL, (uint32_t)p->n_shared,
                                       p->n_shared ? s->d_shared : NULL, w->s_kernel) :
         rain ? g->grid_finish_rain(w->ctx, s->d_acc, r->n_sel, n_cells, d_rain, s->d_means,
                                    s->d_means + n_sel * n_cells, p->n_shared ? d_idx : NULL, (uint32_t)p->n_shared,
                                    p->n_shared ? s->d_shared : NULL, w->s_kernel) :
         storm ? (ladder ? g->grid_finish_storms : g->grid_finish_weighted)(
                     w->ctx, s->d_acc, r->n_sel, n_cells, s->d_means, s->d_means + n_sel * n_cells,
                     p->n_shared ? d_idx : NULL, (uint32_t)p->n_shared, p->n_shared ? s->d_shared : NULL, w->s_kernel)
               : g->grid_finish(w->ctx, s->d_acc, r->n_sel, n_cells, s->d_means, p->n_shared ? d_idx : NULL,
                                (uint32_t)p->n_shared, p->n_shared ? s->d_shared : NULL, w->s_kernel)) != 0 ||
        g->memcpy_d2h(w->ctx, s->h_means, s->d_means, bytes, w->s_kernel) != 0 ||
        (p->n_shared && g->memcpy_d2h(w->ctx, s->h_shared, s->d_shared,
                                      n_sel * p->n_shared * words * sizeof *s->h_shared, w->s_kernel) != 0))
        goto gpu_fail;
    {
        const double t0 = gcn10_now_seconds();

        if (g->stream_sync(w->ctx, w->s_kernel) != 0)
            goto gpu_fail;
        w->t_gpu_wait += gcn10_now_seconds() - t0;
    }
    if (merge_block(r, p, s->h_means, storm || rain ? s->h_means + n_sel * n_cells : NULL,
                    (const uint64_t *)s->h_shared) != 0) {
        wlog(w, "ERROR", true, "out of memory for the shared cells of block %d", in->block_id);
        return -1;
    }
    return 0;

gpu_fail:
    wlog(w, "ERROR", true, "gpu: %s", g->last_error());
    if (w->ctx)
        g->stream_sync(w->ctx, w->s_kernel);
    return -1;
}

/* ---- the rasters, after the last block ---- */

struct grid_file {
    gcn10_tiff_writer *tif;
    const uint8_t *data;
    atomic_int failed;
};

struct grid_tile_job {
    struct run *run;
    struct grid_file *file;
    struct gcn10_job_group *group;
    int ty;
};

/* one tile row of one raster */
static void grid_tile_row(void *arg)
{
    struct grid_tile_job *j = arg;
    const int nx = j->run->grid.nx, ny = j->run->grid.ny;
    uint8_t z[TILE * TILE + TILE * TILE / 1000 + 64];       /* >= compressBound(65536) */
    const int across = gcn10_tiff_tiles_across(j->file->tif);
    const int vh = ny - j->ty * TILE < TILE ? ny - j->ty * TILE : TILE;

    for (int tx = 0; tx < across; tx++) {
        const int vw = nx - tx * TILE < TILE ? nx - tx * TILE : TILE;
        const size_t n = gcn10_deflate_tile(j->file->data + (size_t)j->ty * TILE * (size_t)nx + (size_t)tx * TILE,
                                            (size_t)nx, vw, vh, j->run->deflate_level, z, sizeof z);

        if (n == 0 || gcn10_tiff_put_tile(j->file->tif, tx, j->ty, z, n) != 0) {
            atomic_store(&j->file->failed, 1);
            break;
        }
    }
    gcn10_job_group_done(j->group);
}

/* The rasters, each through a temporary name and rename (the writer's), and the closing console line.  The exit code: 0,
 * or 1 when a raster could not be written. */
static int grid_finish(struct run *r, gcn10_log *log0)
{
    struct gcn10_grid_result *t = r->grid_result;
    const gcn10_grid *gr = &r->grid;
    const size_t plane = (size_t)gr->nx * (size_t)gr->ny, words = (size_t)t->words, width = (size_t)t->n_sel * words;
    const int n_storms = t->n_cnq;
    const int per = 1 + n_storms, n_files = per * r->n_sel;             /* files per selected raster, and of the run */
    const double gt[6] = { gr->xmin, gr->dx, 0.0, gr->ymax, 0.0, -gr->dy };
    const int down = (gr->ny + TILE - 1) / TILE;
    /* file per q: the mean of q; file per q + 1 + k (storms only): the runoff-equivalent raster of q for storm k */
    struct grid_file files[(1 + GCN10_MAX_STORMS) * GCN10_N_RASTERS];
    struct grid_tile_job *jobs;
    struct gcn10_job_group group;
    char msg[PATH_MAX + 256], err[PATH_MAX + 256] = "", names[GCN10_MAX_STORMS * 16 + 64];
    size_t empty = 0;
    int rc = 0;

    /* the shared cells' sums become bytes by the rule of the kernels */
    for (size_t i = 0; i < t->cap; i++)
        if (t->key[i] != NO_KEY)
            for (int q = 0; q < r->n_sel; q++) {
                const uint64_t *v = &t->pair[i * width + words * (size_t)q];
                uint8_t of_layer[GCN10_MAX_RAINS], cn[GCN10_MAX_RAINS];

                t->raster[(size_t)q * plane + t->key[i]] = mean_of(v[0], v[1]);
                if (r->rain_on) {           /* per layer, with the table of the cell's own byte in it */
                    for (int k = 0; k < n_storms; k++)
                        of_layer[k] = r->rain_layer[k][t->key[i]];
                    gcn10_rains_cell(v, n_storms, of_layer, r->rain_q, cn);
                }
                for (int k = 0; k < n_storms; k++)
                    t->cnq[((size_t)k * (size_t)r->n_sel + (size_t)q) * plane + t->key[i]] =
                        r->rain_on ? cn[k] : (uint8_t)gcn10_runoff_cn(v[0], v[1], v[2 + k], r->runoff_q[k]);
            }
    for (size_t c = 0; c < plane; c++) {
        int q = 0;

        while (q < r->n_sel && t->raster[(size_t)q * plane + c] == GCN10_NODATA)
            q++;
        empty += q == r->n_sel;
    }
    for (int c = 0; c < 2; c++) {
        char dir[64];

        if (!(r->cond_mask & (1u << c)))
            continue;
        snprintf(dir, sizeof dir, "cn_grid_%s", gcn10_conds[c]);
        if (mkdir(dir, 0755) != 0 && errno != EEXIST) {
            snprintf(msg, sizeof msg, "failed to create output directory %s", dir);
            gcn10_log_message(log0, "ERROR", msg, true);
            return 1;
        }
    }
    jobs = calloc((size_t)n_files * (size_t)down, sizeof *jobs);
    if (!jobs) {
        gcn10_log_message(log0, "ERROR", "grid: out of memory for the tile jobs", true);
        return 1;
    }
    memset(files, 0, sizeof files);
    gcn10_job_group_init(&group);
    for (int fi = 0; fi < n_files; fi++) {
        const int q = fi / per, k = r->sel[q];
        char path[PATH_MAX];

        if (fi % per == 0)
            snprintf(path, sizeof path, "cn_grid_%s/cn_%s_%s.tif", gcn10_conds[k / 9], gcn10_hcs[(k % 9) / 3],
                     gcn10_arcs[k % 3]);
        else if (r->rain_on && r->n_rains == 1)
            snprintf(path, sizeof path, "cn_grid_%s/cnq_%s_%s_rain.tif", gcn10_conds[k / 9], gcn10_hcs[(k % 9) / 3],
                     gcn10_arcs[k % 3]);
        else if (r->rain_on)
            snprintf(path, sizeof path, "cn_grid_%s/cnq_%s_%s_rain%d.tif", gcn10_conds[k / 9], gcn10_hcs[(k % 9) / 3],
                     gcn10_arcs[k % 3], fi % per);
        else
            snprintf(path, sizeof path, "cn_grid_%s/cnq_%s_%s_p%u.tif", gcn10_conds[k / 9], gcn10_hcs[(k % 9) / 3],
                     gcn10_arcs[k % 3], (unsigned)r->runoff_q[fi % per - 1][100]);
        files[fi].data = fi % per == 0 ? t->raster + (size_t)q * plane
                         : t->cnq + ((size_t)(fi % per - 1) * (size_t)r->n_sel + (size_t)q) * plane;
        files[fi].tif = gcn10_tiff_create(path, gr->nx, gr->ny, gt, t->esa ? gcn10_raster_georef(t->esa) : NULL, err,
                                          sizeof err);
        if (files[fi].tif && r->nodata >= 0 && gcn10_tiff_set_nodata(files[fi].tif, r->nodata) != 0) {
            snprintf(err, sizeof err, "write error: cannot place the GDAL tags of %s", path);
            gcn10_tiff_abort(files[fi].tif);
            files[fi].tif = NULL;
        }
        if (!files[fi].tif) {
            gcn10_log_message(log0, "ERROR", err, true);
            rc = -1;
            continue;
        }
        for (int ty = 0; ty < down; ty++) {
            struct grid_tile_job *j = &jobs[(size_t)fi * (size_t)down + (size_t)ty];

            j->run = r;
            j->file = &files[fi];
            j->group = &group;
            j->ty = ty;
            gcn10_job_group_add(&group, 1);
            gcn10_pool_submit(r->pool, grid_tile_row, j);
        }
    }
    gcn10_job_group_wait(&group);
    gcn10_job_group_destroy(&group);
    free(jobs);
    for (int fi = 0; fi < n_files; fi++) {
        if (!files[fi].tif)
            continue;
        if (atomic_load(&files[fi].failed)) {
            gcn10_tiff_abort(files[fi].tif);
            snprintf(err, sizeof err, "write error: a tile of raster %d of the grid could not be written",
                     r->sel[fi / per]);
        }
        else if (gcn10_tiff_finish(files[fi].tif, err, sizeof err) == 0) {
            continue;
        }
        gcn10_log_message(log0, "ERROR", err, true);
        rc = -1;
    }
    if (rc != 0) {
        gcn10_log_message(log0, "ERROR", "grid: the rasters could not be written", true);
        return 1;
    }
    if (r->storm_on) {
        /* every storm's suffix: "cnq_<hc>_<arc>_p2500.tif, _p5000.tif" */
        int at = snprintf(names, sizeof names, "cnq_<hc>_<arc>_p%u.tif", (unsigned)r->runoff_q[0][100]);

        for (int k = 1; k < n_storms; k++)
            at += snprintf(names + at, sizeof names - (size_t)at, ", _p%u.tif", (unsigned)r->runoff_q[k][100]);
        snprintf(msg, sizeof msg, "grid: %d blocks, %d rasters of %d x %d cells, %zu cells without a valid pixel, under "
                 "cn_grid_<cond>/: cn_<hc>_<arc>.tif (mean) and %s (runoff-equivalent)", t->blocks,
                 r->n_sel, gr->nx, gr->ny, empty, names);
    }
    else if (r->rain_on && r->n_rains == 1)
        snprintf(msg, sizeof msg, "grid: %d blocks, %d rasters of %d x %d cells, %zu cells without a valid pixel, under "
                 "cn_grid_<cond>/: cn_<hc>_<arc>.tif (mean) and cnq_<hc>_<arc>_rain.tif (runoff-equivalent)", t->blocks,
                 r->n_sel, gr->nx, gr->ny, empty);
    else if (r->rain_on) {
        /* every raster's suffix: "cnq_<hc>_<arc>_rain1.tif, _rain2.tif" */
        int at = snprintf(names, sizeof names, "cnq_<hc>_<arc>_rain1.tif");

        for (int k = 2; k <= n_storms; k++)
            at += snprintf(names + at, sizeof names - (size_t)at, ", _rain%d.tif", k);
        snprintf(msg, sizeof msg, "grid: %d blocks, %d rasters of %d x %d cells, %zu cells without a valid pixel, under "
                 "cn_grid_<cond>/: cn_<hc>_<arc>.tif (mean) and %s (runoff-equivalent)", t->blocks, r->n_sel, gr->nx,
                 gr->ny, empty, names);
    }
    else
        snprintf(msg, sizeof msg, "grid: %d blocks, %d rasters of %d x %d cells, %zu cells without a valid pixel, under "
                 "cn_grid_<cond>/", t->blocks, r->n_sel, gr->nx, gr->ny, empty);
    gcn10_log_message(log0, "INFO", msg, true);
    return 0;
}

static void grid_plan_free(struct block_in *in)
{
    gcn10_grid_plan_free(&in->gplan);
}

const struct gcn10_mode gcn10_mode_grid = {
    .plan_block = grid_plan_input, .plan_free = grid_plan_free, .block = grid_block,
    .block_unreadable = grid_block_unreadable, .worker_teardown = grid_teardown,
    .finish = grid_finish, .end = grid_end,
};
