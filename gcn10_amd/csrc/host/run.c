/* run.c -- gcn10_run, the program of src/main.c:58-203: resolve what the run is to do, require what it needs of the
 * GPU library, plan its workers, load its inputs, let the workers (pipeline.c) run, report.  Every step is a function
 * below; a step that fails has said why and returns non-zero, and gcn10_run frees whatever there is by then.
 */
#include "pipeline_internal.h"

#include <limits.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/resource.h>
#include <unistd.h>

#define now_seconds gcn10_now_seconds

/* What the config and the command line ask for, and every combination that is refused, before any GPU is opened.  A
 * write run unless verify, zonal, aggregate, grid or runoff_rain is asked for: they refuse each other, so r->mode is set
 * once. */
static int resolve(struct run *r)
{
    const gcn10_run_options *opt = &r->opt;
    const char *sink = getenv("GCN10_SINK");
    const char *why = NULL;
    char err[2048] = "";

    r->mode = &gcn10_mode_write;
    r->out_dir = "cn_rasters";
    r->out_name = "cn";
    if (!opt->config_path) {
        fprintf(stderr, "[rank 0] missing -c/--config <file>; see 'gcn10 -h' for usage.\n");   /* src/main.c:103-106 */
        return 1;
    }
    if (gcn10_config_parse(opt->config_path, &r->cfg, err, sizeof err) != 0) {
        fprintf(stderr, "%s\n", err);                   /* src/config.c:52, 109-111 */
        return 1;
    }
    /* the rasters of this run: all 18 unless "lookups" / "conditions" (config or command line) say less */
    r->cond_mask = r->cfg.cond_mask;
    r->table_mask = r->cfg.table_mask;
    if ((opt->lookups && gcn10_parse_lookups(opt->lookups, &r->table_mask) != 0) ||
        (opt->conditions && gcn10_parse_conditions(opt->conditions, &r->cond_mask) != 0)) {
        fprintf(stderr, "[rank 0] bad --lookups / --conditions value; see 'gcn10 -h' for usage.\n");
        return 1;
    }
    if (opt->compress && gcn10_parse_compress(opt->compress, &r->cfg.compress) != 0) {
        fprintf(stderr, "[rank 0] bad value for compress: '%s' (deflate or lzw)\n", opt->compress);
        return 1;
    }
    if (r->cfg.compress == GCN10_COMPRESS_LZW && r->cfg.gpu_deflate == 0) {
        fprintf(stderr, "[rank 0] bad value for compress: 'lzw' with gpu_deflate=0 (LZW tiles are encoded on the GPU "
                        "only; there is no host LZW encoder)\n");
        return 1;
    }
    if (opt->overview_resampling &&
        gcn10_parse_overview_resampling(opt->overview_resampling, &r->cfg.overview_resampling) != 0) {
        fprintf(stderr, "[rank 0] bad value for overview_resampling: '%s' (nearest or average)\n",
                opt->overview_resampling);
        return 1;
    }
    if (opt->cog)
        r->cfg.cog = 1;
    if (opt->stats)
        r->cfg.stats = 1;
    if (opt->nodata && gcn10_parse_nodata(opt->nodata, &r->cfg.nodata) != 0) {
        fprintf(stderr, "[rank 0] bad value for nodata: '%s' (none or an integer 0..255)\n", opt->nodata);
        return 1;
    }
    if (opt->verify)
        r->cfg.verify = 1;
    r->verify = r->cfg.verify != 0;
    if (r->verify && opt->overwrite) {
        fprintf(stderr, "[rank 0] --verify writes nothing and cannot be combined with --overwrite\n");
        return 1;
    }
    if (r->verify)
        r->mode = &gcn10_mode_verify;
    if (r->cfg.cog && r->cfg.gpu_deflate == 0) {
        fprintf(stderr, "[rank 0] bad value for cog: '1' with gpu_deflate=0 (overviews are built and encoded on the GPU "
                        "only; there is no host fallback)\n");
        return 1;
    }
    for (int k = 0; k < GCN10_N_RASTERS; k++)
        if ((r->cond_mask >> (k / 9)) & 1u && (r->table_mask >> (k % 9)) & 1u)
            r->sel[r->n_sel++] = k;
    /* runoff rasters under a rainfall raster: everything it cannot go with, before any of those starts */
    if (gcn10_runoff_start(r) != 0)
        return 1;
    if (r->runoff_on)
        r->mode = &gcn10_mode_runoff;
    /* a rainfall raster, or several ("rains"): the runs they cannot go with, tested before any of them starts, and their
     * unit; the rasters themselves are read once the grid is known (gcn10_grid_start) */
    if (opt->rain) {
        free(r->cfg.rain);
        r->cfg.rain = strdup(opt->rain);
    }
    if (opt->rains) {
        free(r->cfg.rains);
        r->cfg.rains = strdup(opt->rains);
    }
    if (opt->rain_unit) {
        free(r->cfg.rain_unit);
        r->cfg.rain_unit = strdup(opt->rain_unit);
    }
    r->rains_key = r->cfg.rains != NULL;
    r->rain_on = r->cfg.rain != NULL || r->rains_key;
    if (r->cfg.rain_unit && !r->rain_on) {
        fprintf(stderr, "[rank 0] rain_unit needs rain\n");
        return 1;
    }
    if (r->rains_key && r->cfg.rain) {
        fprintf(stderr, "[rank 0] rains cannot be combined with rain\n");
        return 1;
    }
    if (r->rain_on) {
        const char *key = r->rains_key ? "rains" : "rain";
        int factor = r->cfg.aggregate;

        if (opt->aggregate && gcn10_parse_aggregate(opt->aggregate, &factor) != 0)
            factor = 0;                     /* a bad value is reported below, as without rain */
        if (r->verify)
            why = "cannot be combined with --verify";
        else if (factor)
            why = "cannot be combined with aggregate";
        else if (r->cfg.zonal || opt->zonal)
            why = "cannot be combined with --zonal";
        else if (opt->storm || r->cfg.storm)
            why = "cannot be combined with storm";
        else if (opt->storms || r->cfg.storms)
            why = "cannot be combined with storms";
        else if (!opt->grid && !r->cfg.grid)
            why = "needs --grid";
        if (why) {
            fprintf(stderr, "[rank 0] %s %s\n", key, why);
            return 1;
        }
        if (!r->rains_key) {
            r->n_rains = 1;
            r->rain_file[0] = r->cfg.rain;
        }
        else if (gcn10_parse_rains(r->cfg.rains, &r->rains_copy, r->rain_file, &r->n_rains) != 0) {
            fprintf(stderr, "[rank 0] bad value for rains: '%s' (file1[:file2...]: 1 to %d files)\n", r->cfg.rains,
                    GCN10_MAX_RAINS);
            return 1;
        }
        r->rain_unit = 1.0;
        r->rain_lambda = 0.2;
        if (r->cfg.rain_unit && gcn10_parse_rain_unit(r->cfg.rain_unit, &r->rain_unit, &r->rain_lambda) != 0) {
            fprintf(stderr, "[rank 0] bad value for rain_unit: '%s' (unit[,lambda]: 0 < unit, 255 unit <= 650 mm, 0 <= "
                            "lambda < 1)\n", r->cfg.rain_unit);
            return 1;
        }
    }
    /* a rainfall raster under the zones: what it needs and cannot go with, its unit, and the raster itself -- it carries
     * its own grid, so it is read here, before anything starts */
    if (opt->zone_rain) {
        free(r->cfg.zone_rain);
        r->cfg.zone_rain = strdup(opt->zone_rain);
    }
    if (opt->zone_rain_unit) {
        free(r->cfg.zone_rain_unit);
        r->cfg.zone_rain_unit = strdup(opt->zone_rain_unit);
    }
    if (opt->zone_rains) {
        free(r->cfg.zone_rains);
        r->cfg.zone_rains = strdup(opt->zone_rains);
    }
    r->zone_rains_key = r->cfg.zone_rains != NULL;
    r->zone_rain_on = r->cfg.zone_rain != NULL || r->zone_rains_key;
    if (r->cfg.zone_rain_unit && !r->zone_rain_on) {
        fprintf(stderr, "[rank 0] zone_rain_unit needs zone_rain\n");
        return 1;
    }
    if (r->zone_rains_key && r->cfg.zone_rain) {
        fprintf(stderr, "[rank 0] zone_rains cannot be combined with zone_rain\n");
        return 1;
    }
    if (r->zone_rain_on) {
        const char *key = r->zone_rains_key ? "zone_rains" : "zone_rain";

        if (!r->cfg.zonal && !opt->zonal)
            why = "needs --zones";
        else if (opt->storm || r->cfg.storm)
            why = "cannot be combined with storm";
        else if (opt->storms || r->cfg.storms)
            why = "cannot be combined with storms";
        if (why) {
            fprintf(stderr, "[rank 0] %s %s\n", key, why);
            return 1;
        }
        if (!r->zone_rains_key) {
            r->n_zone_rains = 1;
            r->zone_rain_file[0] = r->cfg.zone_rain;
        }
        else if (gcn10_parse_rains(r->cfg.zone_rains, &r->zone_rains_copy, r->zone_rain_file, &r->n_zone_rains) != 0) {
            fprintf(stderr, "[rank 0] bad value for zone_rains: '%s' (file1[:file2...]: 1 to %d files)\n", r->cfg.zone_rains,
                    GCN10_MAX_RAINS);
            return 1;
        }
        r->zone_rain_unit = 1.0;
        r->zone_rain_lambda = 0.2;
        if (r->cfg.zone_rain_unit &&
            gcn10_parse_rain_unit(r->cfg.zone_rain_unit, &r->zone_rain_unit, &r->zone_rain_lambda) != 0) {
            fprintf(stderr, "[rank 0] bad value for zone_rain_unit: '%s' (unit[,lambda]: 0 < unit, 255 unit <= 650 mm, 0 <= "
                            "lambda < 1)\n", r->cfg.zone_rain_unit);
            return 1;
        }
        if (r->zone_rains_key
                ? gcn10_zone_rains_load(r->zone_rain_file, r->n_zone_rains, &r->zone_rain_grid, r->zone_rain_layer, err,
                                        sizeof err) != 0
                : gcn10_zone_rain_load(r->cfg.zone_rain, &r->zone_rain_grid, &r->zone_rain_layer[0], err, sizeof err) != 0) {
            fprintf(stderr, "[rank 0] %s\n", err);
            return 1;
        }
        r->zone_rain_q = malloc(256 * sizeof *r->zone_rain_q);
        if (!r->zone_rain_q) {
            fprintf(stderr, "[rank 0] out of memory for the tables of the rainfall raster\n");
            return 1;
        }
        gcn10_rain_tables(r->zone_rain_unit, r->zone_rain_lambda, r->zone_rain_q);
    }
    /* a zonal run: refused combinations and the zone file */
    if (opt->zones) {
        free(r->cfg.zones_shp_path);
        r->cfg.zones_shp_path = strdup(opt->zones);
    }
    if (opt->zonal)
        r->cfg.zonal = 1;
    r->zonal = r->cfg.zonal != 0;
    if (r->zonal) {
        gcn10_outer_from_env(&r->outer_rank, &r->outer_size);
        if (!r->cfg.zones_shp_path || !*r->cfg.zones_shp_path)
            why = "zonal=1 needs the zone polygons: zones_shp_path=<file.shp> or --zones <file.shp>";
        else if (opt->overwrite)
            why = "--zonal writes no raster and cannot be combined with --overwrite";
        else if (r->verify)
            why = "--zonal cannot be combined with --verify";
        else if (r->outer_size > 1)
            why = "--zonal runs as one process: merging tables across launcher ranks is not supported";
        if (why)
            fprintf(stderr, "[rank 0] %s\n", why);
        if (why || gcn10_zonal_start(r) != 0)
            return 1;
        r->mode = &gcn10_mode_zonal;
    }
    /* an aggregate run: the factor, and the refused combinations */
    if (opt->aggregate && gcn10_parse_aggregate(opt->aggregate, &r->cfg.aggregate) != 0) {
        fprintf(stderr, "[rank 0] bad value for aggregate: '%s' (0 or an integer 2..256)\n", opt->aggregate);
        return 1;
    }
    r->aggregate = r->cfg.aggregate;
    /* a design storm: its runoff table, and the runs it cannot go with */
    if (opt->storm) {
        if (gcn10_parse_storm(opt->storm, &r->cfg.storm_p, &r->cfg.storm_lambda) != 0) {
            fprintf(stderr, "[rank 0] bad value for storm: '%s' (P[,lambda]: 0 < P <= 650 mm, 0 <= lambda < 1)\n",
                    opt->storm);
            return 1;
        }
        free(r->cfg.storm);
        r->cfg.storm = strdup(opt->storm);
    }
    if (opt->storms) {
        if (gcn10_parse_storms(opt->storms, r->cfg.storms_p, &r->cfg.n_storms, &r->cfg.storms_lambda) != 0) {
            fprintf(stderr, "[rank 0] bad value for storms: '%s' (P1[:P2...][,lambda]: 1 to 8 rising depths, 0 < P <= 650 "
                            "mm, 0 <= lambda < 1)\n", opt->storms);
            return 1;
        }
        free(r->cfg.storms);
        r->cfg.storms = strdup(opt->storms);
    }
    r->storms_key = r->cfg.storms != NULL;
    r->storm_on = r->cfg.storm != NULL || r->storms_key;
    if (r->storm_on) {
        const char *const key = r->storms_key ? "storms" : "storm";

        if (r->storms_key && r->cfg.storm)
            why = "cannot be combined with storm";
        else if (r->verify)
            why = "cannot be combined with --verify";
        else if (r->aggregate)
            why = "cannot be combined with aggregate (use --grid with cells of f pixels)";
        else if (!r->zonal && !opt->grid && !r->cfg.grid)
            why = "needs --grid or --zones";
        if (why) {
            fprintf(stderr, "[rank 0] %s %s\n", key, why);
            return 1;
        }
        r->n_storms = r->storms_key ? r->cfg.n_storms : 1;
        r->storm_lambda = r->storms_key ? r->cfg.storms_lambda : r->cfg.storm_lambda;
        for (int k = 0; k < r->n_storms; k++) {
            r->storm_p[k] = r->storms_key ? r->cfg.storms_p[k] : r->cfg.storm_p;
            gcn10_runoff_table(r->storm_p[k], r->storm_lambda, r->runoff_q[k]);
        }
    }
    if (r->aggregate) {
        if (gcn10_aggregate_start(r) != 0)
            return 1;
        r->mode = &gcn10_mode_aggregate;
    }
    /* a grid run: the grid, the refused combinations, the result of the run */
    if (opt->grid) {
        free(r->cfg.grid);
        r->cfg.grid = strdup(opt->grid);
    }
    r->grid_on = r->cfg.grid != NULL;
    if (r->grid_on) {
        if (gcn10_grid_start(r) != 0)
            return 1;
        r->mode = &gcn10_mode_grid;
    }
    r->null_sink = sink && strcmp(sink, "null") == 0;
    /* Rows per strip.  Rounds 2 and 3 ran 768 rows (three tile rows of a 36000-px block = 423 tile positions, one round
     * of the fused statistics pass's 512 workgroup slots); larger strips lost end to end to the coarser hand-over between
     * kernels, copy-back and file writes (profiles/r02/strip_rows_ab.txt, profiles/r03/pipeline_strip_rows_48_blocks.txt).
     * With the kernels of the end of round 3 a 768-row strip is 0.11-0.22 ms of GPU work, and what a strip costs
     * besides -- a dozen HIP calls, three launch prologues, 18 writes -- weighs more: 2304 rows (nine tile rows),
     * 72 blocks, steady state, patchy blocks: null sink 0.0074 -> 0.0063 s per block, files 0.0107 -> 0.0092;
     * noisy blocks unchanged within the noise (profiles/r03/sink_sweep2_patches_72_blocks.txt,
     * strip_rows3_natural_72_blocks.txt).  3072 is no better; pinned memory grows with the strip (1.9 GB per GPU). */
    r->strip_rows = r->cfg.strip_rows > 0 ? (r->cfg.strip_rows + TILE - 1) / TILE * TILE : DEFAULT_STRIP_ROWS;
    if (r->strip_rows > MAX_STRIP_ROWS)     /* a strip's compressed-tile arena must stay below 4 GiB (32-bit offsets) */
        r->strip_rows = MAX_STRIP_ROWS;
    r->deflate_level = r->cfg.deflate_level;
    r->gpu_deflate = r->cfg.gpu_deflate != 0;
    r->lzw = r->cfg.compress == GCN10_COMPRESS_LZW;
    r->cog = r->cfg.cog != 0;
    r->ov_average = r->cfg.overview_resampling == GCN10_OVERVIEW_AVERAGE;
    r->stats = r->cfg.stats != 0;
    r->nodata = r->cfg.nodata;
    r->fused = r->cfg.gpu_deflate == 2 && !r->lzw;     /* the fused encoder is DEFLATE-only */
    if (r->runoff_on)
        r->fused = false;       /* ... and makes curve numbers: the runoff strips go through the per-raster encoder */
    if (r->aggregate) {
        /* the aggregated rasters are made on the device and go through the per-raster GPU encoder, whatever
         * "gpu_deflate" says; they carry neither overviews nor statistics */
        r->gpu_deflate = true;
        r->cog = r->stats = false;
    }
    if (r->grid_on)
        r->cog = r->stats = false;      /* the grid rasters are encoded on the host and carry neither */
    r->gpu_inflate = r->cfg.gpu_inflate != 0;
    r->direct_io = r->cfg.direct_io != 0 || (getenv("GCN10_DIRECT_IO") && atoi(getenv("GCN10_DIRECT_IO")) != 0);
    r->prefetch = r->cfg.prefetch_blocks != 0 && !(getenv("GCN10_PREFETCH_BLOCKS") && atoi(getenv("GCN10_PREFETCH_BLOCKS")) == 0);
    r->nbuf = DEFAULT_NBUF;
    if (getenv("GCN10_STRIP_BUFFERS")) {
        int n = atoi(getenv("GCN10_STRIP_BUFFERS"));

        r->nbuf = n < 2 ? 2 : (n > MAX_NBUF ? MAX_NBUF : n);
    }
    r->drain_lag = 2;
    r->event_sleep_us = getenv("GCN10_EVENT_SLEEP_US") ? atoi(getenv("GCN10_EVENT_SLEEP_US")) : 50;
    if (getenv("GCN10_DRAIN_LAG"))
        r->drain_lag = atoi(getenv("GCN10_DRAIN_LAG"));
    if (r->drain_lag < 1)
        r->drain_lag = 1;
    if (r->drain_lag > r->nbuf - 1)
        r->drain_lag = r->nbuf - 1;     /* the strip whose buffer is reused next must have been drained */
    return 0;
}

/* The GPU library, and the optional entry points of it that the modes of this run need. */
static int require(struct run *r)
{
    const struct gcn10_gpu_api *g;
    char err[2048] = "", agg[48], grid[600], storm[600], rain[PATH_MAX + 8], zrain[PATH_MAX + 16], *rains = NULL, *zrains = NULL;
    char rrain[PATH_MAX + 16];
    int rc = 0;

    r->gpu = g = gcn10_gpu_api_get(err, sizeof err);
    if (!g) {
        fprintf(stderr, "[rank 0] %s\n", err);
        return 1;
    }
    snprintf(agg, sizeof agg, "aggregate=%d", r->aggregate);
    snprintf(grid, sizeof grid, "grid=%s", r->grid_on ? r->cfg.grid : "");
    snprintf(storm, sizeof storm, "%s=%s", r->storms_key ? "storms" : "storm",
             r->storms_key ? r->cfg.storms : r->storm_on ? r->cfg.storm : "");
    snprintf(rain, sizeof rain, "rain=%s", r->rain_on && !r->rains_key ? r->cfg.rain : "");
    if (r->rains_key) {                     /* up to eight paths: as long as the key's value */
        const size_t cap = strlen(r->cfg.rains) + 8;

        if (!(rains = malloc(cap))) {
            fprintf(stderr, "[rank 0] out of memory\n");
            return 1;
        }
        snprintf(rains, cap, "rains=%s", r->cfg.rains);
    }
    snprintf(rrain, sizeof rrain, "runoff_rain=%s", r->runoff_on ? r->cfg.runoff_rain : "");
    snprintf(zrain, sizeof zrain, "zone_rain=%s", r->zone_rain_on && !r->zone_rains_key ? r->cfg.zone_rain : "");
    if (r->zone_rains_key) {
        const size_t cap = strlen(r->cfg.zone_rains) + 16;

        if (!(zrains = malloc(cap))) {
            free(rains);
            fprintf(stderr, "[rank 0] out of memory\n");
            return 1;
        }
        snprintf(zrains, cap, "zone_rains=%s", r->cfg.zone_rains);
    }
    {
        /* the pair histogram's soil codes are asked for where a mode counts pairs, and must be as many as its bins */
        const bool pairs = (r->stats || r->zonal) && g->pair_histogram_codes &&
                           g->pair_histogram_codes(r->hist_codes) == GCN10_PAIR_HIST_BINS;
        const struct { bool on, present; const char *symbol, *needed_by; } needs[] = {
            { r->cog, g->overview_nearest && g->overview_average, "gcn10_gpu_overview_*", "cog=1" },
            { r->stats, g->pair_histogram && pairs, "gcn10_gpu_pair_histogram", "stats=1" },
            { r->zone_rain_on && !r->zone_rains_key, g->set_rain_tables && g->zonal_sums_rain, "gcn10_gpu_zonal_sums_rain",
              zrain },
            { r->zone_rains_key, g->set_rain_tables && g->zonal_sums_rains, "gcn10_gpu_zonal_sums_rains", zrains },
            { r->zonal, g->zonal_pair_histogram && pairs, "gcn10_gpu_zonal_pair_histogram", "zonal=1" },
            { r->aggregate != 0, g->aggregate != NULL, "gcn10_gpu_aggregate", agg },
            { r->grid_on && r->storm_on && !r->storms_key,
              g->set_weights && g->grid_sums_weighted && g->grid_finish_weighted, "gcn10_gpu_grid_sums_weighted", storm },
            { r->grid_on && r->storms_key, g->set_weight_tables && g->grid_sums_storms && g->grid_finish_storms,
              "gcn10_gpu_grid_sums_storms", storm },
            { r->rain_on && !r->rains_key, g->set_rain_tables && g->grid_sums_rain && g->grid_finish_rain,
              "gcn10_gpu_grid_sums_rain", rain },
            { r->rains_key, g->set_rain_tables && g->grid_sums_rains && g->grid_finish_rains,
              "gcn10_gpu_grid_sums_rains", rains },
            { r->grid_on, g->grid_sums && g->grid_finish, "gcn10_gpu_grid_sums", grid },
            { r->verify, g->verify_strip && g->verify_buffers, "gcn10_gpu_verify_strip", "verify=1" },
            { r->lzw, g->lzw_strip && g->lzw_arena_bound, "gcn10_gpu_lzw_strip", "compress=lzw" },
            { r->runoff_on, g->set_cell_byte_tables && g->runoff_strip, "gcn10_gpu_runoff_strip", rrain },
        };

        for (size_t i = 0; rc == 0 && i < sizeof needs / sizeof needs[0]; i++)
            if (needs[i].on && !needs[i].present) {
                fprintf(stderr, "[rank 0] %s lacks %s (needed by %s)\n", gcn10_gpu_library_path(), needs[i].symbol,
                        needs[i].needed_by);
                rc = 1;
            }
    }
    free(rains);
    free(zrains);
    if (rc)
        return rc;
    r->inflate_codecs = GCN10_CODEC_DEFLATE | GCN10_CODEC_RAW;
    if (r->cfg.gpu_inflate_lzw && g->inflate_codecs && (g->inflate_codecs() & GCN10_CODEC_LZW))
        r->inflate_codecs |= GCN10_CODEC_LZW;
    return 0;
}

/* GPUs to use, and worker threads ("ranks") per GPU: two workers per GPU keep the device busy while one of them opens
 * files, reads the soil window or finishes its GeoTIFFs (measured +25 % blocks per second). */
static int plan_workers(struct run *r)
{
    const int n_dev = r->gpu->device_count();
    const int per_gpu = r->cfg.workers_per_gpu > 0 ? r->cfg.workers_per_gpu : 2;
    int gpus = r->opt.gpus > 0 ? r->opt.gpus : (r->cfg.gpus > 0 ? r->cfg.gpus : n_dev);

    if (n_dev <= 0) {
        fprintf(stderr, "[rank 0] no MI355X (gfx950) device visible; the CN path has no CPU fallback\n");
        return 1;
    }
    r->n_physical = n_dev;
    if (getenv("GCN10_REHEARSE_GPUS") && atoi(getenv("GCN10_REHEARSE_GPUS")) > 0) {
        /* dress rehearsal of an N-GPU node on the devices that are here: N logical GPUs with
         * per_gpu workers each, one I/O pool, N "timing gpu" lines; logical GPU d runs on device
         * d % n_dev.  Same code path as a real node from the block queue to the per-GPU lines. */
        r->n_devices = atoi(getenv("GCN10_REHEARSE_GPUS"));
        if (r->opt.gpus > 0 && r->opt.gpus < r->n_devices)
            r->n_devices = r->opt.gpus;
        r->n_workers = r->n_devices * per_gpu;
    }
    else if (getenv("GCN10_OVERSUBSCRIBE")) {    /* tests: N workers on however few GPUs there are */
        r->n_devices = n_dev;
        r->n_workers = gpus;
    }
    else {
        if (gpus > n_dev)
            gpus = n_dev;
        r->n_devices = gpus;
        r->n_workers = gpus * per_gpu;
    }
    if (r->n_workers > 64)
        r->n_workers = 64;
    gcn10_outer_from_env(&r->outer_rank, &r->outer_size);
    r->workers = calloc((size_t)r->n_workers, sizeof *r->workers);
    return r->workers ? 0 : 1;
}

static void log0_line(struct run *r, const char *level, bool console, const char *fmt, ...)
    __attribute__((format(printf, 4, 5)));
static void log0_line(struct run *r, const char *level, bool console, const char *fmt, ...)
{
    char msg[8192];
    va_list ap;

    va_start(ap, fmt);
    vsnprintf(msg, sizeof msg, fmt, ap);
    va_end(ap);
    gcn10_log_message(r->workers[0].log, level, msg, console);
}

static void on_lookup_row_error(void *user, const char *message)
{
    gcn10_log_message(user, "ERROR", message, true);       /* src/cn.c:61, 71, 81 */
}

/* the nine lookup tables, once (the reference re-reads one per raster, src/cn.c:261) */
static int load_tables(struct run *r)
{
    /* only the lookups this run produces are read (the reference reads one per raster it
     * writes, src/cn.c:261); a table that is not selected stays "no value" (255, src/cn.c:36-40) */
    for (int k = 0; k < 9; k++) {
        const char *hc = gcn10_hcs[k / 3], *arc = gcn10_arcs[k % 3];
        int rc;

        if (!(r->table_mask & (1u << k))) {
            for (int lc = 0; lc < 256; lc++)
                for (int sg = 0; sg < 5; sg++)
                    r->tables[k][lc][sg] = 255;
            continue;
        }
        rc = gcn10_load_lookup_table(r->cfg.lookup_table_path, hc, arc, r->tables[k], on_lookup_row_error,
                                     r->workers[0].log);
        if (rc == 0)
            continue;
        log0_line(r, "ERROR", true, "%s %s/default_lookup_%s_%s.csv",
                  rc == -2 ? "empty lookup table" :                   /* src/cn.c:44 */
                  rc == -3 ? "lookup table path too long:" :          /* :23 */
                             "cannot open lookup table",              /* :30 */
                  r->cfg.lookup_table_path, hc, arc);
        return 1;
    }
    return 0;
}

/* Logs, the block index, the ids of the run's blocks, the lookup tables; then no more workers than blocks, this
 * process's share of the blocks under a launcher, the I/O pool and the verify run's list. */
static int load(struct run *r)
{
    const gcn10_run_options *opt = &r->opt;
    char err[2048] = "";
    gcn10_log *log0 = gcn10_log_open(r->cfg.log_dir, r->outer_rank * r->n_workers);   /* init_logging(rank), src/main.c:129 */
    long ncpu = sysconf(_SC_NPROCESSORS_ONLN);
    int nthreads = r->cfg.io_threads > 0 ? r->cfg.io_threads : (int)(ncpu > 2 ? ncpu - 1 : 1);

    r->workers[0].log = log0;
    log0_line(r, "INFO", true,
              "starting processing with %d gpu workers (ranks)\n"
              "check rank_0.log in the log directory for detailed progress\n"
              "config loaded:\n"
              "  hysogs_data_path   = %s\n"
              "  esa_data_path      = %s\n"
              "  blocks_shp_path    = %s\n"
              "  lookup_table_path  = %s\n"
              "  log_dir            = %s",                /* src/main.c:114-125 */
              r->n_workers, r->cfg.hysogs_data_path, r->cfg.esa_data_path, r->cfg.blocks_shp_path,
              r->cfg.lookup_table_path, r->cfg.log_dir);
    for (int i = 1; i < r->n_workers; i++)
        r->workers[i].log = gcn10_log_open(r->cfg.log_dir, r->outer_rank * r->n_workers + i);
    for (int i = 0; i < r->n_workers; i++) {
        r->workers[i].run = r;
        r->workers[i].index = i;
        r->workers[i].rank = r->outer_rank * r->n_workers + i;
    }

    /* the block index is needed for bboxes in either mode */
    if (gcn10_blocks_open(r->cfg.blocks_shp_path, &r->blocks, err, sizeof err) != 0) {
        gcn10_log_message(log0, "ERROR", err, true);    /* "ogr open failed: ..." */
        if (!opt->blocks_file) {
            log0_line(r, "ERROR", true, "failed to read shapefile %s", r->cfg.blocks_shp_path);  /* src/main.c:143 */
            return 1;
        }
        /* list mode: every block then fails like the reference's per-block OGROpen (src/cn.c:156-160) */
    }
    if (opt->blocks_file) {
        r->block_ids = gcn10_read_block_list(opt->blocks_file, &r->n_blocks);
        if (!r->block_ids)
            log0_line(r, "ERROR", true, "cannot open block list file %s", opt->blocks_file);    /* src/raster.c:33 */
        if (!r->block_ids || !r->n_blocks) {
            log0_line(r, "ERROR", true, "no ids found in %s", opt->blocks_file);                /* src/main.c:135 */
            return 1;
        }
    }
    else {
        /* every "ID" of the shapefile (what get_all_blocks is meant to return,
         * src/raster.c:94-101; its `ids[*n_blocks++]` never gets that far) */
        r->n_blocks = r->blocks.n;
        r->block_ids = malloc((size_t)(r->n_blocks ? r->n_blocks : 1) * sizeof *r->block_ids);
        if (r->block_ids)
            memcpy(r->block_ids, r->blocks.id, (size_t)r->n_blocks * sizeof *r->block_ids);
        if (!r->block_ids || !r->n_blocks) {
            log0_line(r, "ERROR", true, "no blocks found in %s", r->cfg.blocks_shp_path);       /* src/main.c:148 */
            return 1;
        }
    }
    if (load_tables(r) != 0)
        return 1;

    log0_line(r, "INFO", true, "processing %d blocks %s", r->n_blocks,
              opt->blocks_file ? "from list file" : "from shapefile");      /* src/main.c:165-167 */
    for (int k = 0; r->storm_on && k < r->n_storms; k++) {      /* one line per storm, in the order given */
        int threshold = 1;

        while (threshold < 100 && r->runoff_q[k][threshold] == 0)
            threshold++;
        log0_line(r, "INFO", true, "storm: P = %.17g mm, lambda = %.17g, threshold CN %d (the smallest curve number that "
                  "sheds water)", r->storm_p[k], r->storm_lambda, threshold);
    }
    for (int j = 0; r->rain_on && j < r->n_rains; j++) {    /* two lines per raster, in the order given */
        const size_t n = (size_t)r->grid.nx * (size_t)r->grid.ny;
        const uint8_t *rain = r->rain_layer[j];
        unsigned lo = 255, hi = 0;
        size_t dry = 0;
        char tag[16] = "rain";

        if (r->n_rains > 1)
            snprintf(tag, sizeof tag, "rain[%d]", j + 1);
        for (size_t c = 0; c < n; c++) {
            lo = rain[c] < lo ? rain[c] : lo;
            hi = rain[c] > hi ? rain[c] : hi;
            dry += rain[c] == 0;
        }
        log0_line(r, "INFO", true, "%s: %s, %d x %d cells, unit = %.17g mm, lambda = %.17g", tag, r->rain_file[j],
                  r->grid.nx, r->grid.ny, r->rain_unit, r->rain_lambda);
        log0_line(r, "INFO", true, "%s: depths %u..%u counts, %zu cells without rain", tag, lo, hi, dry);
    }
    for (int j = 0; r->zone_rain_on && j < r->n_zone_rains; j++) {      /* two lines per raster, in the order given */
        const gcn10_grid *zg = &r->zone_rain_grid;
        const size_t n = (size_t)zg->nx * (size_t)zg->ny;
        const uint8_t *rain = r->zone_rain_layer[j];
        unsigned lo = 255, hi = 0;
        size_t dry = 0;
        char tag[24] = "zone_rain";

        if (r->n_zone_rains > 1)
            snprintf(tag, sizeof tag, "zone_rain[%d]", j + 1);
        for (size_t c = 0; c < n; c++) {
            lo = rain[c] < lo ? rain[c] : lo;
            hi = rain[c] > hi ? rain[c] : hi;
            dry += rain[c] == 0;
        }
        log0_line(r, "INFO", true, "%s: %s, %d x %d cells of %.17g x %.17g from (%.17g, %.17g), unit = %.17g mm, "
                  "lambda = %.17g", tag, r->zone_rain_file[j], zg->nx, zg->ny, zg->dx, zg->dy, zg->xmin, zg->ymax,
                  r->zone_rain_unit, r->zone_rain_lambda);
        log0_line(r, "INFO", true, "%s: depths %u..%u counts, %zu cells without rain", tag, lo, hi, dry);
    }
    if (r->runoff_on) {
        const gcn10_grid *zg = &r->runoff_grid;

        log0_line(r, "INFO", true, "runoff_rain: %s, %d x %d cells of %.17g x %.17g from (%.17g, %.17g), unit = %.17g mm, "
                  "lambda = %.17g, 1 count = %u/100 mm", r->cfg.runoff_rain, zg->nx, zg->ny, zg->dx, zg->dy, zg->xmin,
                  zg->ymax, r->runoff_rain_unit, r->runoff_lambda, r->runoff_u);
    }
    if (r->n_workers > r->n_blocks) {       /* no worker (and no pinned memory) without a block */
        for (int i = r->n_blocks > 0 ? r->n_blocks : 1; i < r->n_workers; i++) {
            gcn10_log_close(r->workers[i].log);
            r->workers[i].log = NULL;
        }
        r->n_workers = r->n_blocks > 0 ? r->n_blocks : 1;
    }

    /* under mpirun / srun every process takes the reference's static share of the
     * list, i = rank, rank + size, ... (src/main.c:171), and feeds its own GPUs */
    if (r->outer_size > 1) {
        int kept = 0;

        for (int i = r->outer_rank; i < r->n_blocks; i += r->outer_size)
            r->block_ids[kept++] = r->block_ids[i];
        log0_line(r, "INFO", true, "process %d of %d: %d of %d blocks", r->outer_rank, r->outer_size, kept, r->n_blocks);
        r->n_blocks = kept;
    }

    r->pool = gcn10_pool_create(nthreads > 64 ? 64 : nthreads);
    if (!r->pool) {
        log0_line(r, "ERROR", true, "cannot start the tile compression threads");
        return 1;
    }
    if (r->verify) {
        pthread_mutex_init(&r->verify_mu, NULL);
        r->verify_failed = malloc((size_t)(r->n_blocks > 0 ? r->n_blocks : 1) * sizeof *r->verify_failed);
        r->verify_failed_cap = r->verify_failed ? r->n_blocks : 0;
        log0_line(r, "INFO", true, "verify: nothing is written; the rasters that exist are compared with the "
                  "values computed now");
    }
    return 0;
}

/* what the workers of GPU d (d < 0: of all GPUs) have added up */
struct worker_sums {
    int workers, blocks;
    double busy, read, gpu_wait, sink_wait, soil, create, finish, device, in_wait, in_busy, zone_plan, zone_accum;
    double cpu, in_cpu;
    long win_gpu, win_gpu_lzw, win_host;
    const struct worker *first;
};

static struct worker_sums sum_workers(const struct run *r, int d)
{
    struct worker_sums s = { 0 };

    for (int i = 0; i < r->n_workers; i++) {
        const struct worker *w = &r->workers[i];

        if (d >= 0 && w->index % r->n_devices != d)
            continue;
        if (!s.first)
            s.first = w;
        s.workers++;
        s.blocks += w->blocks_done;
        s.busy += w->busy_seconds;
        s.read += w->t_read;
        s.gpu_wait += w->t_gpu_wait;
        s.sink_wait += w->t_sink_wait;
        s.soil += w->t_soil;
        s.create += w->t_create;
        s.finish += w->t_finish;
        s.device += w->t_device;
        s.in_wait += w->t_in_wait;
        s.in_busy += w->t_in_busy;
        s.zone_plan += w->t_zone_plan;
        s.zone_accum += w->t_zone_accum;
        s.cpu += w->cpu_seconds;
        s.in_cpu += w->in_cpu_seconds;
        s.win_gpu += w->n_win_gpu;
        s.win_gpu_lzw += w->n_win_gpu_lzw;
        s.win_host += w->n_win_host;
    }
    return s;
}

/* CPU seconds of the whole process (all threads): against the wall time this says whether the host side is what
 * bounds the run (a cgroup CPU quota shows as user + system ~ quota x wall); then by kind of thread -- the rest is the
 * HIP runtime's own threads and the main thread -- and the I/O pool's by kind of job */
static void report_cpu(struct run *r, const struct worker_sums *all, double t_start)
{
    struct rusage ru;
    struct gcn10_job_cpu job[4];            /* append, gate, finish, host deflate */
    const double io = gcn10_pool_cpu_seconds(r->pool);
    double user, sys;
    uint64_t hits = 0, misses = 0;
    size_t held = 0;

    if (getrusage(RUSAGE_SELF, &ru) != 0)
        return;
    user = (double)ru.ru_utime.tv_sec + ru.ru_utime.tv_usec * 1e-6;
    sys = (double)ru.ru_stime.tv_sec + ru.ru_stime.tv_usec * 1e-6;
    log0_line(r, "INFO", false, "timing: host cpu seconds: user %.3f, system %.3f, over %.3f s wall (%.3f per block); "
              "voluntary / involuntary context switches %ld / %ld; pinned host memory allocated %.1f MB; "
              "peak resident set %.1f MB", user, sys, now_seconds() - t_start,
              all->blocks > 0 ? (user + sys) / all->blocks : 0.0, ru.ru_nvcsw, ru.ru_nivcsw,
              (double)atomic_load(&r->pinned_bytes) / 1e6, (double)ru.ru_maxrss / 1e3);
    log0_line(r, "INFO", false, "timing: host cpu seconds by thread: encoder workers %.3f, input threads %.3f, "
              "i/o pool %.3f, others (HIP runtime, main) %.3f", all->cpu, all->in_cpu, io,
              user + sys - all->cpu - all->in_cpu - io);
    gcn10_sink_job_cpu(r->pool, job);
    log0_line(r, "INFO", false, "timing: i/o pool cpu seconds by job: appending a raster's strip %.3f (%ld), "
              "waiting for a strip's bytes %.3f (%ld), finishing files %.3f (%ld), host deflate %.3f (%ld), "
              "reading and decoding inputs %.3f", job[0].seconds, job[0].n, job[1].seconds, job[1].n, job[2].seconds,
              job[2].n, job[3].seconds, job[3].n,
              io - job[0].seconds - job[1].seconds - job[2].seconds - job[3].seconds);
    gcn10_tiff_cache_stats(&hits, &misses, &held);
    log0_line(r, "INFO", false, "timing: decoded-chunk cache (soil strips): %llu hits, %llu misses, %.1f MB held",
              (unsigned long long)hits, (unsigned long long)misses, (double)held / 1e6);
}

/* every "timing" line of the log */
static void report(struct run *r, double t_start)
{
    const struct worker_sums all = sum_workers(r, -1);
    double first = 0.0, rate = 0.0;
    char extras[48];                        /* the GDAL tags of the outputs */

    if (r->zonal)
        log0_line(r, "INFO", false, "timing: zonal: host seconds building spans %.3f (%.4f per block, on the input side), "
                  "adding histograms up %.3f", all.zone_plan, all.blocks > 0 ? all.zone_plan / all.blocks : 0.0,
                  all.zone_accum);
    for (int i = 0; i < r->n_workers; i++) {
        const struct worker *w = &r->workers[i];

        /* from the moment the first worker had its GPU, buffers and files ready: what a long run sees per block */
        if (w->t_first_block > 0.0 && (first == 0.0 || w->t_first_block < first))
            first = w->t_first_block;
        /* blocks per second of every worker after its first block, added up: the rate a long run sees */
        if (w->in_seq > 1 && w->t_last_done > w->t_first_done)
            rate += (double)(w->in_seq - 1) / (w->t_last_done - w->t_first_done);
    }
    if (rate > 0.0)
        log0_line(r, "INFO", false, "timing: steady state %.4f s per block (%.2f blocks per second: every worker's blocks "
                  "after its first, which pays for buffers, pinning and workspaces)", 1.0 / rate, rate);
    snprintf(extras, sizeof extras, "%s", r->stats ? ", stats" : "");
    if (r->nodata >= 0)
        snprintf(extras + strlen(extras), sizeof extras - strlen(extras), ", nodata %d", r->nodata);
    log0_line(r, "INFO", false, "timing: %d blocks, %.3f s wall (%.3f s after start-up), %d gpu worker(s)%s%s%s%s; worker seconds: "
              "in blocks %.3f, reading landcover %.3f, waiting for gpu %.3f, waiting for sink %.3f, "
              "soil window %.3f, creating outputs %.3f, finishing outputs %.3f, device setup %.3f, "
              "waiting for input %.3f; input thread seconds: %.3f%s",
              all.blocks, now_seconds() - t_start, first > 0.0 ? now_seconds() - first : 0.0, r->n_workers,
              r->null_sink ? ", null sink" : "",
              r->lzw ? ", gpu lzw" : r->gpu_deflate ? (r->fused ? ", fused gpu deflate" : ", gpu deflate") : ", host zlib",
              r->gpu_inflate ? ", gpu inflate of deflate landcover" : "", extras, all.busy, all.read, all.gpu_wait,
              all.sink_wait, all.soil, all.create, all.finish, all.device, all.in_wait, all.in_busy,
              r->prefetch ? " (one block ahead of the encoder)" : " (in turn with the encoder)");
    log0_line(r, "INFO", false, "timing: landcover windows: %ld through the gpu decoder (of them %ld with lzw chunks), "
              "%ld through the host reader", all.win_gpu, all.win_gpu_lzw, all.win_host);
    report_cpu(r, &all, t_start);
    /* one line per GPU: when a node's GPUs are not equally busy, these tell a slow device or PCIe
     * root complex (waiting for gpu) from a slow NUMA node or file system (reading, waiting for sink) */
    for (int d = 0; d < r->n_devices; d++) {
        const struct worker_sums s = sum_workers(r, d);

        if (s.first)
            log0_line(r, "INFO", false, "timing gpu %d (pci %s, numa node %d): %d worker(s), %d blocks, worker seconds: "
                      "in blocks %.3f, reading landcover %.3f, waiting for gpu %.3f, waiting for sink %.3f, "
                      "soil window %.3f, finishing outputs %.3f", d, s.first->pci_bus[0] ? s.first->pci_bus : "?",
                      s.first->numa_node, s.workers, s.blocks, s.busy, s.read, s.gpu_wait, s.sink_wait, s.soil, s.finish);
    }
}

int gcn10_run(const gcn10_run_options *opt)
{
    struct run *r = calloc(1, sizeof *r);
    gcn10_log *log0 = NULL;
    int exit_code = 1, loaded;
    const double t_start = now_seconds();

    if (!r) {
        fprintf(stderr, "out of memory\n");
        return 1;
    }
    r->opt = *opt;
    if (resolve(r) != 0 || require(r) != 0 || plan_workers(r) != 0)
        goto done;
    loaded = load(r);
    log0 = r->workers[0].log;
    if (loaded != 0)
        goto done;

    atomic_store(&r->next_block, 0);
    atomic_store(&r->fatal, 0);
    for (int i = 0; i < r->n_workers; i++)
        if (pthread_create(&r->workers[i].thread, NULL, gcn10_worker_main, &r->workers[i]) != 0) {
            gcn10_log_message(log0, "ERROR", "cannot start a gpu worker thread", true);
            atomic_store(&r->fatal, 1);
            r->n_workers = i;
            break;
        }
    for (int i = 0; i < r->n_workers; i++)
        pthread_join(r->workers[i].thread, NULL);      /* MPI_Barrier, src/main.c:187 */

    log0_line(r, "INFO", true, "processed %d blocks on %d ranks", r->n_blocks, r->n_workers);  /* src/main.c:191 */
    if (r->outer_size > 1) {
        if (r->mode->leave_part)
            r->mode->leave_part(r);
        gcn10_closing_barrier(r, log0);     /* MPI_Barrier + rank 0's summary, src/main.c:187-194 */
    }
    /* the mode's result, closing line and exit code; an error that ended the run or a result that lacks a block is 1 */
    exit_code = r->mode->finish ? r->mode->finish(r, log0) : 0;
    report(r, t_start);
    if (atomic_load(&r->fatal) || atomic_load(&r->incomplete))
        exit_code = 1;

done:
    gcn10_pool_destroy(r->pool);
    for (int i = 1; r->workers && i < r->n_workers; i++)
        gcn10_log_close(r->workers[i].log);
    gcn10_log_close(log0);                              /* finalize_logging, src/main.c:197 */
    free(r->workers);
    free(r->verify_failed);
    if (r->mode->end)
        r->mode->end(r);
    for (int j = 0; j < GCN10_MAX_RAINS; j++)
        free(r->zone_rain_layer[j]);
    free(r->zone_rains_copy);
    free(r->zone_rain_q);
    free(r->rains_copy);
    free(r->block_ids);
    gcn10_blocks_free(&r->blocks);
    gcn10_config_free(&r->cfg);
    free(r);
    return exit_code;
}
