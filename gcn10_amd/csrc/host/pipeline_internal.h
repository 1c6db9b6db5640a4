/* pipeline_internal.h -- the worker and run state shared by run.c (the run's steps), pipeline.c (workers, a block's
 * strips), sink.c (strip buffers, sink jobs), pipeline_input.c (landcover input through the GPU decoder), launcher.c and
 * the kinds of run, and what the writer and the verifier have in common: the chunk stager (stage.c) and the overview
 * levels (levels.c).  A run is of one kind -- write (pipeline.c), aggregate.c, verify.c, zonal.c, grid.c or
 * runoff_raster.c -- and each
 * is a struct gcn10_mode beside its code; resolve() (run.c) leaves the run's in run.mode and the driver calls through
 * it.  Every kind takes a staged block over with gcn10_block_take, the one reader of the decoder's status words. */
#ifndef GCN10_PIPELINE_INTERNAL_H
#define GCN10_PIPELINE_INTERNAL_H

#include "gcn10_host.h"
#include "host_internal.h"

#include <pthread.h>
#include <stdatomic.h>
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

enum { TILE = 256, MAX_NBUF = 8, DEFAULT_NBUF = 4, DEFAULT_STRIP_ROWS = 2304, MAX_STRIP_ROWS = 4096 };

struct run;
struct worker;
struct gcn10_verify_state;
struct gcn10_zonal_state;
struct gcn10_zonal_table;
struct gcn10_grid_state;
struct gcn10_grid_result;
struct gcn10_runoff_state;

/* ---- stage.c: chunks as they lie in the files -> pinned ring -> device, for gcn10_gpu_inflate_tiles ---- */

/* bytes a chunk of nbytes takes in the staging buffers and on the device: 16-byte aligned, and 16 zero bytes behind
 * it (the decoder's bit reader may look a few bytes ahead) */
size_t gcn10_chunk_slot(uint32_t nbytes);
/* the decoder's job for chunk c: its bytes at in_off of the compressed buffer, its pixels to dst_off of the output */
void gcn10_inflate_job_from_chunk(gcn10_inflate_tile *j, const struct gcn10_chunk_ref *c, uint64_t in_off,
                                  uint64_t dst_off);

/* the jobs of one gcn10_gpu_inflate_tiles call and their status words, host (pinned) and device, and the stager's
 * word on each job's chunk (gcn10_stager_stage's bad[]; pinned like the rest, so there is one way to fail) */
struct gcn10_job_list {
    gcn10_inflate_tile *h_jobs, *d_jobs;
    uint32_t *h_status, *d_status;
    int *bad;
    size_t cap;
};
/* room for n jobs; the first `keep` host entries stay.  Nothing may be in flight on the lists.  0, or a device error */
int gcn10_job_list_ensure(const struct gcn10_gpu_api *g, gcn10_gpu_ctx *ctx, struct gcn10_job_list *l, size_t n,
                          size_t keep);
void gcn10_job_list_free(const struct gcn10_gpu_api *g, gcn10_gpu_ctx *ctx, struct gcn10_job_list *l);

/* A ring of pinned buffers of one size on one context: buffer k is filled while the copy of buffer k - 1 to the device
 * is in flight.  One thread uses a stager.  Every call returns 0 or a device error (gpu->last_error() has the text). */
enum { GCN10_STAGER_MAX = 3 };
struct gcn10_stager {
    const struct gcn10_gpu_api *gpu;
    gcn10_gpu_ctx *ctx;
    gcn10_pool *pool;                       /* reads the chunks; NULL: the calling thread does */
    atomic_llong *pinned_bytes;             /* the run's count of pinned memory asked for */
    int n;
    size_t cap;                             /* bytes of one buffer */
    uint8_t *h[GCN10_STAGER_MAX];
    gcn10_event_t ev[GCN10_STAGER_MAX];
    bool busy[GCN10_STAGER_MAX];            /* a copy out of the buffer was issued and not yet waited for */
    /* the batch being read: pool jobs take slices of [next, end) in turn */
    struct gcn10_job_group reads;
    const struct gcn10_chunk_ref *chunks;
    const gcn10_inflate_tile *jobs;
    int *bad;
    uint8_t *dst;
    uint64_t base;
    atomic_size_t next;
    size_t end;
};
/* n_buffers events, and buffers of `bytes` (0: none before the first gcn10_stager_ensure) */
int gcn10_stager_setup(struct gcn10_stager *s, const struct gcn10_gpu_api *g, gcn10_gpu_ctx *ctx, gcn10_pool *pool,
                       atomic_llong *pinned_bytes, int n_buffers, size_t bytes);
void gcn10_stager_teardown(struct gcn10_stager *s);
/* buffers of at least `bytes`: waits for the copies in flight, then reallocates */
int gcn10_stager_ensure(struct gcn10_stager *s, size_t bytes);
/* buffer k free to be written (its last copy has finished); a copy out of buffer k has been issued on `stream` */
int gcn10_stager_take(struct gcn10_stager *s, int k);
int gcn10_stager_sent(struct gcn10_stager *s, int k, gcn10_stream_t stream);
/* the caller has waited for the stream of the copies: every buffer is free */
void gcn10_stager_idle(struct gcn10_stager *s);
/* The n chunks to d_comp + jobs[i].in_off (in_off ascending, a gcn10_chunk_slot apart), as many per buffer as fit,
 * copied on `stream`.  bad[i] = 0: staged; 1: its bytes cannot be read (zeros are staged); 2: larger than a buffer
 * (nothing is staged).  The other chunks go on either way. */
int gcn10_stager_stage(struct gcn10_stager *s, const struct gcn10_chunk_ref *chunks, const gcn10_inflate_tile *jobs,
                       size_t n, uint8_t *d_comp, gcn10_stream_t stream, int *bad);

/* one rotating set of strip buffers */
struct strip_buf {
    uint8_t *h_out[GCN10_N_RASTERS];        /* pinned */
    uint8_t *d_out[GCN10_N_RASTERS];
    gcn10_event_t ev_h2d, ev_kernel, ev_d2h, ev_meta;
    /* GPU-side DEFLATE: compressed tiles of all 18 rasters of the strip */
    uint8_t *d_arena, *h_arena;             /* h_arena pinned */
    size_t arena_cap;                       /* device arena: the encoder's worst case      */
    size_t h_arena_cap;                     /* pinned arena: an eighth of it (>= 32 MB)    */
    uint8_t *h_spill;                       /* pageable stand-in when a strip needs more   */
    const uint8_t *h_tiles;                 /* where this strip's streams are: arena or spill */
    size_t h_tiles_used;                    /* ... and how many bytes of them the encoder produced */
    uint32_t *d_table, *h_table;            /* [18][tiles][2]; h_table pinned */
    unsigned long long *d_cursor, *h_cursor;
    const uint8_t **d_ptrs;                 /* device array of the 18 d_out pointers */
    struct gcn10_job_group jobs;            /* sink jobs of the strip currently held by this buffer */
    bool d2h_issued;
    int y0, rows;                           /* strip held */
    struct worker *owner;
};

/* One landcover block on its way from the files to the encoder.  Filled by the worker's input thread
 * (pipeline_input.c) while the worker encodes the block before it: window arithmetic, soil window and index
 * maps, the landcover window staged through pinned memory and decoded / untiled into d_block.  Everything in
 * it belongs to the input thread while state == FILLING and to the worker while READY. */
enum { IN_FREE = 0, IN_FILLING = 1, IN_READY = 2, IN_END = 3 };
enum { N_IN = 2 };                          /* the block being encoded + the one being staged */
enum { N_RING = 3 };                        /* pinned staging buffers of the input thread */
enum { RING_BYTES = 64 << 20 };             /* ... each; a block of DEFLATE landcover is 2-3 of them (the verifier's too) */

struct block_in {
    int state;                              /* IN_*; guarded by worker.in_mu */
    int block_id;
    int outcome;                            /* 0 = encode it; 1 = skipped (logged, like a failed load_raster,
                                               src/cn.c:188-203); -1 = an error the reference answers with MPI_Abort */
    int xoff, yoff, W, H, hsx, hsy;
    double gt[6];
    uint8_t *h_coarse;                      /* pinned: soil window, index maps */
    int32_t *h_ci, *h_cj;
    size_t h_coarse_cap, h_ci_cap, h_cj_cap;
    uint8_t *d_coarse;
    int32_t *d_ci, *d_cj;
    size_t coarse_cap, ci_cap, cj_cap;
    uint8_t *d_block;                       /* the landcover window, W x H, row major */
    size_t block_cap;
    uint8_t *d_comp;                        /* the window's chunks as they lie in the files (compressed or raw) */
    size_t d_comp_cap;
    struct gcn10_job_list jl;               /* the decoder's jobs and their status words */
    size_t n_inflate;                       /* chunks whose status must be looked at (0: host reader) */
    gcn10_event_t ev_ready;                 /* recorded behind everything the block needs on the device */
    /* the block's output files (src/cn.c:236-360: directories, names, the trailing-underscore rule), created by
     * the input side while the block before is encoded: 18 open + truncate calls are 5-10 ms per block */
    gcn10_tiff_writer *tifs[GCN10_N_RASTERS];
    bool tifs_ok;                           /* all of the run's rasters have their file */
    int out_W, out_H;                       /* the rasters in them: the window's, unless the mode's plan_block says */
    double out_gt[6];                       /* otherwise (aggregate.c: the block's grid of cells) */
    /* the mode's plan of the block (plan_block, plan_free): the zones' spans and items over it (zonal.c, zones.c), its
     * owned pixels and grid of cells (aggregate.c), its cell rectangle, maps and shared cells (grid.c) */
    gcn10_zone_plan zplan;
    gcn10_aggregate_geom agg;
    gcn10_grid_plan gplan;
    gcn10_grid_plan zr_gplan;               /* zone_rain: the block on the raster's grid, */
    gcn10_zone_rain_plan zr_cut;            /* ... and the zones' spans cut at its depth changes */
    gcn10_zone_rains_plan zrs_cut;          /* zone_rains: the spans cut where the byte of any layer changes */
    gcn10_grid_plan rr_gplan;               /* runoff_rain: the block on the raster's grid, every pixel of the window */
};

struct worker {
    struct run *run;
    int rank;                               /* "rank" in the logs: outer_rank * n_workers + index */
    int index;                              /* worker index in this process; GPU = index % n_devices */
    pthread_t thread;
    gcn10_log *log;
    gcn10_gpu_ctx *ctx;
    gcn10_stream_t s_kernel, s_d2h;
    gcn10_raster *esa, *soil;
    size_t buf_px;                          /* capacity of one strip buffer, pixels */
    size_t buf_tiles;                       /* ... and in 256x256 tiles */
    int strip_rows;                         /* rows per strip of the current block */
    int n_cus;                              /* compute units of this worker's GPU */
    struct strip_buf buf[MAX_NBUF];         /* the first run->nbuf are in use */
    atomic_bool failed;                     /* a sink job of the current block failed */
    bool fused;                             /* this worker's tables allow the fused encoder */
    /* input side: a thread of its own (prefetch_blocks=1) or the worker itself, in turn */
    pthread_t in_thread;
    bool in_thread_started;
    gcn10_gpu_ctx *in_ctx;                  /* the input thread's own context on the same device */
    gcn10_stream_t s_in;
    struct block_in in[N_IN];
    pthread_mutex_t in_mu;
    pthread_cond_t in_cv;
    bool in_stop;                           /* the worker is going away: the input thread must not wait for it */
    struct gcn10_stager ring;               /* pinned: chunks (or host-decoded rows) on their way to the device */
    int blocks_done;
    int in_seq;                             /* blocks taken from the input side so far: slot = in_seq % N_IN */
    int device;                             /* the GPU this worker drives */
    int numa_node;                          /* ... and the NUMA node it hangs off (-1 = unknown) */
    char pci_bus[64];
    double busy_seconds;
    double cpu_seconds, in_cpu_seconds;        /* CPU time of the worker's thread and of its input thread */
    double t_first_block;                   /* when this worker started its first block */
    double t_first_done, t_last_done;       /* when it finished its first / its last block */
    double t_gpu_wait, t_sink_wait;         /* where the worker thread's time goes */
    double t_create, t_finish, t_device, t_in_wait;
    double t_read, t_soil, t_in_busy;       /* ... and the input thread's */
    /* COG output: the overview phase's device buffers, and the order in which strips reach the files (a COG takes
     * tile data in file order only: the gate jobs of a worker's strips append their extents in turn) */
    uint8_t *d_ov;                          /* nearest: one level's landcover; average: the whole pyramid */
    size_t ov_cap;
    int32_t *d_ov_idx;                      /* nearest: a level's ci then cj */
    size_t ov_idx_cap;
    void *d_ov_ptrs;                        /* average: per strip of a level, the n_sel raster pointers */
    size_t ov_ptrs_cap;
    pthread_mutex_t gate_mu;
    pthread_cond_t gate_cv;
    long gate_seq, gate_turn;
    /* band statistics (stats=1): the block's pair histogram on the device, and its copy */
    unsigned long long *d_hist, *h_hist;    /* GCN10_PAIR_HIST_SIZE counters; h_hist pinned */
    size_t d_hist_cap, h_hist_cap;
    /* the mode's buffers of this worker, made with its first block, freed by worker_teardown: decode buffers and
     * counters (verify.c), span, item and histogram buffers (zonal.c), map, sum and mean buffers (grid.c) */
    struct gcn10_verify_state *verify;
    struct gcn10_zonal_state *zonal;
    struct gcn10_grid_state *gridst;
    struct gcn10_runoff_state *runoffst;    /* map and cell-byte buffers (runoff_raster.c) */
    /* runoff_rain: what gcn10_run_strips hands gcn10_gpu_runoff_strip in the place of cn_strip, set by the mode around its
     * call (NULL: cn_strip): the block's maps and the bytes of its cell rectangle, on the device */
    const struct gcn10_runoff_strip_args {
        const int32_t *d_cellx, *d_celly;
        const uint8_t *d_cells;
        int ncx, ncy;
    } *runoff;
    double t_zone_plan, t_zone_accum;       /* zonal: seconds of the input side building spans, of the worker adding up */
    long n_win_gpu, n_win_gpu_lzw, n_win_host;  /* landcover windows through the GPU decoder (of them with LZW chunks),
                                                   through the host reader */
};

struct run {
    gcn10_config cfg;
    gcn10_run_options opt;
    const struct gcn10_gpu_api *gpu;
    gcn10_blocks blocks;
    int *block_ids;
    int n_blocks;
    int tables[9][256][5];
    int n_workers;
    struct worker *workers;
    gcn10_pool *pool;
    atomic_llong pinned_bytes;              /* pinned host memory asked for by all workers (allocations; regrowth counts twice) */
    atomic_int next_block;
    atomic_int fatal;                       /* a worker hit an MPI_Abort-class error */
    int strip_rows;                         /* "strip_rows" of the config, rounded up to whole tile rows */
    int nbuf;                               /* strip buffer sets per worker (GCN10_STRIP_BUFFERS, 2..8) */
    int event_sleep_us;                     /* GPU events are waited for with query + sleep (0: the runtime's spinning wait) */
    int drain_lag;                          /* the strip handed to the sink while strip s is submitted: s - drain_lag */
    int deflate_level;
    bool null_sink;                         /* GCN10_SINK=null: no compression, no files */
    bool gpu_deflate;                       /* tiles are encoded on the GPU */
    bool fused;                             /* ... straight from landcover + soil (no CN rasters in HBM) */
    bool lzw;                               /* ... as TIFF LZW streams (compress=lzw: per-raster, never fused) */
    bool gpu_inflate;                       /* DEFLATE landcover tiles are decoded on the GPU */
    unsigned inflate_codecs;                /* GCN10_CODEC_* the read plans hand to the GPU decoder (LZW: gpu_inflate_lzw=1
                                               and a library that decodes it) */
    bool direct_io;                         /* tile data is written with O_DIRECT */
    bool cog;                               /* Cloud Optimized GeoTIFFs with overviews (cog=1) */
    bool ov_average;                        /* ... made by averaging (overview_resampling=average), else nearest */
    atomic_bool cog_logged;                 /* the run log has its COG line */
    bool stats;                             /* GDAL band statistics in every written raster (stats=1) */
    int nodata;                             /* GDAL_NODATA of every written raster, -1 = none (nodata=) */
    uint8_t hist_codes[GCN10_PAIR_HIST_BINS];   /* soil code of each bin of the pair histogram */
    bool prefetch;                          /* input threads stage block N+1 while block N is encoded */
    int n_devices;                          /* GPUs of the run; worker i belongs to GPU i % n_devices */
    int n_physical;                         /* ... and the devices behind them: GPU d is device d % n_physical (all the
                                               same unless GCN10_REHEARSE_GPUS rehearses a bigger node on this one) */
    int outer_rank, outer_size;             /* this process among the processes of an mpirun / srun */
    unsigned cond_mask, table_mask;         /* the rasters this run produces ("conditions" / "lookups") */
    int n_sel;                              /* how many: popcount(cond_mask) * popcount(table_mask) */
    int sel[GCN10_N_RASTERS];               /* their raster indices cond*9 + hc*3 + arc, ascending */
    /* the kind of run, which the driver calls through; and what the config says, for resolve()'s refusals, require()'s
     * table, the modes themselves and sink.c (an aggregate run has no full-resolution strips) */
    const struct gcn10_mode *mode;
    bool verify, zonal, grid_on;
    int aggregate;                          /* the factor f, 0 = none */
    atomic_int incomplete;                  /* a block could not be read and the run's one result lacks it: exit code 1 */
    /* verify=1: nothing is written; what the workers found */
    atomic_int verify_n_ok, verify_n_bad, verify_n_missing, verify_n_unchecked;    /* files; overview levels */
    pthread_mutex_t verify_mu;
    int *verify_failed;                     /* ids of the blocks with a bad or missing file, in the order found */
    int verify_n_failed, verify_failed_cap;
    /* zonal=1: nothing is written but the table of composite curve numbers per zone (zonal.c) */
    gcn10_zones zones;
    struct gcn10_zonal_table *zonal_table;
    /* aggregate=<f>: no 10 m raster is written but every selected raster's area means over f x f pixels, under
     * cn_rasters_<cond><out_suffix> (aggregate.c) */
    char out_suffix[16];
    /* grid=...: no 10 m raster is written but every selected raster's means on one model grid, merged over all blocks
     * and written after the last one (grid.c) */
    gcn10_grid grid;
    struct gcn10_grid_result *grid_result;
    /* storm=... or storms=...: the runoff-weighted composites beside the means of a grid or zonal run (runoff.c) */
    bool storm_on;
    bool storms_key;                        /* they come from "storms": named per storm, summed by the _storms calls */
    int n_storms;                           /* how many: 1 with "storm", 1 to GCN10_MAX_STORMS with "storms" */
    double storm_p[GCN10_MAX_STORMS], storm_lambda;
    uint16_t runoff_q[GCN10_MAX_STORMS][256];       /* gcn10_runoff_table of every storm */
    /* rain=... / rains=...: a rainfall depth per cell of the grid, or several, and the runoff-equivalent raster for each
     * beside every mean */
    bool rain_on;
    double rain_unit, rain_lambda;
    bool rains_key;                         /* the rasters come from "rains": summed by the _rains calls */
    int n_rains;                            /* how many: 1 with "rain", 1 to GCN10_MAX_RAINS with "rains" */
    char *rains_copy;                       /* gcn10_parse_rains' copy of the "rains" value */
    const char *rain_file[GCN10_MAX_RAINS]; /* their names: cfg.rain, or pointers into rains_copy */
    uint8_t *rain_layer[GCN10_MAX_RAINS];   /* [ny][nx] each: the counts of every rainfall raster (gcn10_rain_load) */
    uint16_t (*rain_q)[256];                /* [256][256]: gcn10_rain_tables */
    /* zone_rain=...: a rainfall raster under the zones of a zonal run, with its own grid (zonal.c) */
    bool zone_rain_on;
    double zone_rain_unit, zone_rain_lambda;
    gcn10_grid zone_rain_grid;              /* the raster as a grid (gcn10_zone_rain_load) */
    bool zone_rains_key;                    /* the rasters come from "zone_rains": summed by the _rains call */
    int n_zone_rains;                       /* how many: 1 with "zone_rain", 1 to GCN10_MAX_RAINS with "zone_rains" */
    char *zone_rains_copy;                  /* gcn10_parse_rains' copy of the "zone_rains" value */
    const char *zone_rain_file[GCN10_MAX_RAINS];    /* their names: cfg.zone_rain, or pointers into zone_rains_copy */
    uint8_t *zone_rain_layer[GCN10_MAX_RAINS];      /* [ny][nx] each: the counts of every raster, all on zone_rain_grid */
    uint16_t (*zone_rain_q)[256];           /* [256][256]: gcn10_rain_tables */
    /* runoff_rain=...: the runoff depth of every pixel under a rainfall raster, written in the place of the curve numbers
     * (runoff_raster.c) */
    bool runoff_on;
    double runoff_rain_unit, runoff_lambda;
    unsigned runoff_u;                      /* hundredths of a millimetre per count of the written rasters */
    gcn10_grid runoff_grid;                 /* the raster as a grid (gcn10_rain_raster_load) */
    uint8_t *runoff_layer;                  /* [ny][nx]: its counts */
    uint8_t (*runoff_t)[256];               /* [256][256]: gcn10_runoff_bytes of gcn10_rain_tables */
    /* the names of a block's files: <out_dir>_<cond><out_suffix>/<out_name>_<hc>_<arc>_<id>.tif ("cn_rasters" and "cn"
     * unless the mode says otherwise) */
    const char *out_dir, *out_name;
};

double gcn10_now_seconds(void);
void gcn10_wlog(struct worker *w, const char *level, bool console, const char *fmt, ...)
    __attribute__((format(printf, 4, 5)));

/* a GPU library call that failed: one log line with its message, and the caller returns `ret` */
#define GPU_OR_RETURN(w, ret, call)                                                    \
    do {                                                                               \
        if ((call) != 0) {                                                             \
            gcn10_wlog((w), "ERROR", true, "gpu: %s", (w)->run->gpu->last_error());    \
            return (ret);                                                              \
        }                                                                              \
    } while (0)

/* sink.c: device / pinned buffer of at least `need` bytes on context `ctx` (grown by reallocation); -1 and a log line
 * on failure */
int gcn10_ensure_dev_on(struct worker *w, gcn10_gpu_ctx *ctx, void **p, size_t *cap, size_t need);
int gcn10_ensure_pinned_on(struct worker *w, gcn10_gpu_ctx *ctx, void **p, size_t *cap, size_t need);
/* sink.c: the worker's strip buffers, sized for blocks W wide (0, or -1: logged).  gcn10_sink_drain hands the finished
 * strip held by buffer b (none: nothing happens) to the pool's sink jobs, gcn10_sink_wait waits for them; once every
 * strip of a block is drained, gcn10_sink_finish_files closes the block's files (ok) or gives them up.
 * gcn10_sink_job_cpu: the pool's CPU seconds and job counts in appending extents, waiting for a strip's bytes,
 * finishing files and host deflate, in this order. */
struct gcn10_job_cpu {
    double seconds;
    long n;
};
int gcn10_sink_ensure_buffers(struct worker *w, int W);
void gcn10_sink_free_buffers(struct worker *w);
int gcn10_sink_drain(struct worker *w, struct strip_buf *b, gcn10_tiff_writer *tifs[GCN10_N_RASTERS], int W, int H);
void gcn10_sink_wait(struct strip_buf *b);
void gcn10_sink_finish_files(struct worker *w, gcn10_tiff_writer *tifs[GCN10_N_RASTERS], bool ok, int block_id);
void gcn10_sink_job_cpu(gcn10_pool *pool, struct gcn10_job_cpu by_kind[4]);
/* pipeline.c: a worker's thread, from its set-up to its teardown */
void *gcn10_worker_main(void *arg);
/* launcher.c: rank and size of this process under mpirun / srun (0 of 1 without); the launch's name in file names;
 * the closing barrier through <log_dir>/.done_<job>_<rank> and launcher rank 0's line of totals */
void gcn10_outer_from_env(int *rank, int *size);
void gcn10_job_tag(char job[96]);
void gcn10_closing_barrier(struct run *r, gcn10_log *log0);

/* levels.c: the overview levels of a staged block, for the writer and the verifier alike.
 * gcn10_level_nearest: level k by nearest-neighbour sampling, ready as a block of its own -- its landcover in w->d_ov,
 *   its index maps on the device, the tile of its width *Wk prepared (the block's own is gone) -- on s_kernel; *d_cj:
 *   its soil rows (the three are set on failure too, and mean nothing then).  The level's kernels must be done before
 *   the next call.
 * gcn10_levels_average: the pyramid of the selected rasters, levels 1 .. L, from the block's prepared tile, strip_rows
 *   rows at a time; levels[q * L + k - 1]: level k of selected raster q, rows gcn10_level_dim(W, k) apart, in w->d_ov.
 * 0, or -1 (logged). */
int gcn10_level_nearest(struct worker *w, const struct block_in *in, int k, int *Wk, int *Hk, const int32_t **d_cj);
int gcn10_levels_average(struct worker *w, const struct block_in *in, int L, int strip_rows,
                         uint8_t *levels[GCN10_N_RASTERS * GCN10_COG_MAX_LEVELS]);

/* pipeline_input.c: the input side of a worker.
 * gcn10_input_setup / _teardown: context, stream, events, pinned ring of the input side.
 * gcn10_input_start: starts the input thread (prefetch) -- it takes block ids from the run's counter, fills
 *   w->in[] slots in turn and marks them IN_READY (IN_END after the last one).
 * gcn10_input_next: the slot the worker encodes next (waits for it; without a thread, fills it right here);
 *   NULL at the end of the queue.  gcn10_input_release hands the slot back. */
/* pipeline.c: the output files of a block (directories, names, overwrite rule); 0, 1 = a file could not be created
 * (logged like save_raster logs, the block is given up), -1 = an output directory cannot be made (fatal, src/cn.c:250) */
int gcn10_create_outputs(struct worker *w, struct block_in *in);
void gcn10_abort_outputs(struct block_in *in);
/* pipeline.c: the strips of one W x H raster through the run's encoder and the sink (see there); aggregate.c hands it
 * the aggregated rasters as `premade` ones */
int gcn10_run_strips(struct worker *w, int W, int H, const uint8_t *d_block, const int32_t *d_cj,
                     const uint8_t *const *premade, unsigned long long *hist, gcn10_tiff_writer *tifs[GCN10_N_RASTERS]);
/* pipeline.c: a staged block taken over by the worker.  gcn10_block_take: s_kernel waits for the input side's event,
 * then the statuses.  gcn10_block_statuses: where chunks went through the decoder, waits for that event on the host and
 * looks at every status word; the first bad one is logged with the two lines of a failed load_raster.  (The write path
 * calls the second alone, behind its strips: a host wait before them would serialise decode and encode.) */
enum { GCN10_BLOCK_READY = 0, GCN10_BLOCK_UNREADABLE = 1, GCN10_BLOCK_DEVICE_ERROR = -1 };   /* (the last: not logged) */
int gcn10_block_take(struct worker *w, const struct block_in *in);
int gcn10_block_statuses(struct worker *w, const struct block_in *in);
/* pipeline.c: the back half of process_block for the modes that write the block's files: the staged block through the
 * mode's strips, the encoder and the sink (0, also for a block given up as the reference gives it up, or -1) */
int gcn10_encode_block(struct worker *w, struct block_in *in);

/* One kind of run.  A member that is NULL is a step the kind does not have. */
struct gcn10_mode {
    bool writes_block_files;                /* the input side creates the block's files (gcn10_create_outputs) */
    /* input side, behind the staging of a block (own: the block's box): 0, or it is logged and the block's outcome is
     * what it returns (1: given up, -1: the run ends); plan_free: what it left in the slot */
    int (*plan_block)(struct worker *w, struct block_in *in, const double own[4]);
    void (*plan_free)(struct block_in *in);
    int (*block)(struct worker *w, struct block_in *in);    /* a staged block: 0, or -1 for errors that end the run */
    int (*strips)(struct worker *w, struct block_in *in, gcn10_tiff_writer *tifs[GCN10_N_RASTERS]); /* (encode_block's) */
    void (*block_unreadable)(struct worker *w, int block_id);   /* one not staged (NULL: skipped as the reference skips) */
    void (*worker_teardown)(struct worker *w);              /* the worker's buffers of the mode */
    void (*leave_part)(struct run *r);                      /* under a launcher, before the closing barrier */
    int (*finish)(struct run *r, gcn10_log *log0);          /* result and closing line; the exit code: 0, 1, 2 (verify) */
    void (*end)(struct run *r);                             /* frees what its start made */
};
extern const struct gcn10_mode gcn10_mode_write, gcn10_mode_aggregate, gcn10_mode_verify, gcn10_mode_zonal,
    gcn10_mode_grid, gcn10_mode_runoff;
/* run.c's resolve() before it chooses the mode, no GPU opened yet: the refused combinations, the zones, the grid's
 * result; 0, or -1 with a line on stderr and nothing left behind */
int gcn10_aggregate_start(struct run *r);
int gcn10_zonal_start(struct run *r);
int gcn10_grid_start(struct run *r);
/* runoff_raster.c: the keys of a runoff_rain run -- the refusals in the order of gcn10_host.h, the units, the raster and
 * its 256 byte tables; 0 (r->runoff_on says whether the run is one), or -1 with a line on stderr */
int gcn10_runoff_start(struct run *r);
int gcn10_input_setup(struct worker *w);
void gcn10_input_teardown(struct worker *w);
int gcn10_input_start(struct worker *w);
struct block_in *gcn10_input_next(struct worker *w);
void gcn10_input_release(struct worker *w, struct block_in *in);
void gcn10_input_stop(struct worker *w);

#endif
