/* host_internal.h -- declarations shared by the host C files, not part of the ABI. */
#ifndef GCN10_HOST_INTERNAL_H
#define GCN10_HOST_INTERNAL_H

#include "gcn10_gpu.h"
#include "gcn10_host.h"

#include <pthread.h>

struct gcn10_tiff;      /* tiff_internal.h: one open TIFF file (tiff_open.c) */
struct gcn10_tiff *gcn10_tiff_open_reader(const char *path, char *err, size_t errcap);
/* directory `level` of the file (0 = the raster, k = overview k of a COG); *why (optional): GCN10_TIFF_E_* of a NULL */
enum { GCN10_TIFF_E_STRUCTURE = 1, GCN10_TIFF_E_MISSING = 2, GCN10_TIFF_E_NOT_BYTE = 3, GCN10_TIFF_E_NO_IFD = 4 };
struct gcn10_tiff *gcn10_tiff_open_reader_ifd(const char *path, int level, int *why, char *err, size_t errcap);
int gcn10_tiff_reader_samples(const struct gcn10_tiff *t);      /* SamplesPerPixel of the file */
bool gcn10_tiff_reader_has_next(const struct gcn10_tiff *t);    /* another directory follows this one */
int gcn10_tiff_check_chunks(const struct gcn10_tiff *t, uint64_t *index, uint64_t *off, uint64_t *count);
void gcn10_tiff_close_reader(struct gcn10_tiff *t);
void gcn10_tiff_reader_info(const struct gcn10_tiff *t, int *xsize, int *ysize, double gt[6]);
const gcn10_georef *gcn10_tiff_reader_georef(const struct gcn10_tiff *t);
int gcn10_tiff_read_window(struct gcn10_tiff *t, int xoff, int yoff, int xcount, int ycount,
                           uint8_t *dst, size_t dst_stride, char *err, size_t errcap);


/* size of overview level k of a raster n pixels wide or high: ceil(n / 2^k) */
static inline int gcn10_level_dim(int n, int k)
{
    return (int)(((int64_t)n + ((int64_t)1 << k) - 1) >> k);
}

/* pool.c: fixed thread pool (tile compression, tile decode) */
typedef struct gcn10_pool gcn10_pool;
typedef void (*gcn10_job_fn)(void *arg);
gcn10_pool *gcn10_pool_create(int n_threads);
void gcn10_pool_submit(gcn10_pool *p, gcn10_job_fn fn, void *arg);
void gcn10_pool_destroy(gcn10_pool *p);     /* drains the queue first */
double gcn10_pool_cpu_seconds(gcn10_pool *p);   /* CPU time its (live) threads have used so far */
double gcn10_pool_cpu_of(gcn10_pool *p, gcn10_job_fn fn, long *n_jobs);     /* ... in jobs of one kind */
double gcn10_thread_cpu_seconds(void);          /* ... the calling thread */
/* The jobs someone has handed out and waits for: add before a job is submitted, done as the job's last step, wait
 * until every job added is done.  A group may be added to again while it is waited for (a job that hands out more). */
struct gcn10_job_group {
    pthread_mutex_t mu;
    pthread_cond_t cv;
    int pending;
};
void gcn10_job_group_init(struct gcn10_job_group *g);
void gcn10_job_group_destroy(struct gcn10_job_group *g);
void gcn10_job_group_add(struct gcn10_job_group *g, int n);
void gcn10_job_group_done(struct gcn10_job_group *g);
void gcn10_job_group_wait(struct gcn10_job_group *g);
void gcn10_tiff_cache_stats(uint64_t *hits, uint64_t *misses, size_t *bytes);     /* decoded-chunk cache of tiff_cache.c */

/* Like gcn10_tiff_read_window / gcn10_raster_read, with the tiles or strips of the
 * window decoded concurrently on `pool` (NULL = on the calling thread). */
int gcn10_tiff_read_window_mt(struct gcn10_tiff *t, int xoff, int yoff, int xcount, int ycount,
                              uint8_t *dst, size_t dst_stride, gcn10_pool *pool, char *err,
                              size_t errcap);
int gcn10_raster_read_mt(gcn10_raster *r, int xoff, int yoff, int xcount, int ycount, uint8_t *dst,
                         gcn10_pool *pool, char *err, size_t errcap);

/* Read plans: the compressed chunks (tiles or strips) of a window, for decoding on the GPU
 * (gcn10_gpu_inflate_tiles) instead of on the I/O pool. */
struct gcn10_chunk_ref {
    int fd;                     /* file that holds the chunk (stays open while the plan lives) */
    uint64_t file_off;
    uint32_t nbytes;            /* compressed size */
    uint32_t chunk_w, rows;     /* decoded shape */
    uint32_t src_x, src_y;      /* first wanted pixel of the chunk */
    uint32_t copy_w, copy_h;
    uint32_t dst_x, dst_y;      /* where it goes in the window */
    uint32_t flags;             /* GCN10_TILE_RAW | GCN10_TILE_PREDICTOR2 | GCN10_TILE_LZW (gcn10_inflate_tile.flags) */
    uint32_t out_len;           /* bytes the chunk stands for on the device: decoded size, or nbytes of a raw one */
};
struct gcn10_read_plan {
    struct gcn10_chunk_ref *chunks;
    size_t n, cap;
    struct gcn10_tiff **opened; /* VRT sources opened for this plan */
    int n_opened;
    uint64_t covered;           /* pixels of the window the chunks fill; the rest reads as 0 */
    uint32_t max_chunk_bytes;   /* largest decoded DEFLATE chunk (raw chunks need no decode slot) */
    uint64_t staged_bytes;      /* bytes of all chunks as they cross PCIe */
};
/* 0 = planned; 1 = this window is left to the host reader (LZW / PackBits, overlapping mosaic
 * sources, full-width raw strips of a much wider raster ...): use gcn10_raster_read_mt; -1 = error (err is set). */
int gcn10_raster_plan_window(gcn10_raster *r, int xoff, int yoff, int xcount, int ycount,
                             struct gcn10_read_plan *plan, char *err, size_t errcap);
/* the same for the chunk codecs in `codecs` (GCN10_CODEC_* of gcn10_gpu.h): with GCN10_CODEC_LZW, LZW chunks
 * are planned too (flags GCN10_TILE_LZW, plus GCN10_TILE_PREDICTOR2 as the file says), under the rules of
 * DEFLATE chunks; gcn10_raster_plan_window = DEFLATE | RAW */
int gcn10_raster_plan_window_codecs(gcn10_raster *r, int xoff, int yoff, int xcount, int ycount, unsigned codecs,
                                    struct gcn10_read_plan *plan, char *err, size_t errcap);
int gcn10_tiff_plan_window(struct gcn10_tiff *t, int xoff, int yoff, int xcount, int ycount, int dst_x,
                           int dst_y, unsigned codecs, struct gcn10_read_plan *plan, char *err, size_t errcap);
void gcn10_read_plan_free(struct gcn10_read_plan *plan);

/* stats.c: gcn10_raster_histogram over the m nonzero counters of a pair histogram alone -- counter i is n[i] at index
 * at[i] = bin * 256 + landcover -- for callers that turn one pair histogram into many rasters' (zonal.c) */
void gcn10_raster_histogram_sparse(const uint16_t *at, const uint64_t *n, size_t m, const uint8_t codes[16],
                                   const int table[256][5], int drained, uint64_t hist[256]);

/* zones.c: the ownership rule of gcn10_zones_build_plan alone -- the pixels [*x0, *x1) x [*y0, *y1) of a north-up
 * W x H block whose centres lie in own = {minx, miny, maxx, maxy}: own[0] <= px < own[2], own[1] < py <= own[3] */
void gcn10_owned_window(const double gt[6], int W, int H, const double own[4], int *x0, int *x1, int *y0, int *y1);

/* gpuapi.c: include/gcn10_gpu.h bound with dlopen */
struct gcn10_gpu_api {
    bool loaded;
    int (*abi_version)(void);
    int (*device_count)(void);
    int (*init)(int, gcn10_gpu_ctx **);
    void (*destroy)(gcn10_gpu_ctx *);
    const char *(*last_error)(void);
    int (*device_info)(gcn10_gpu_ctx *, char *, size_t, size_t *);
    int (*malloc)(gcn10_gpu_ctx *, size_t, void **);
    int (*free)(gcn10_gpu_ctx *, void *);
    int (*host_alloc)(gcn10_gpu_ctx *, size_t, void **);
    int (*host_free)(gcn10_gpu_ctx *, void *);
    int (*memcpy_h2d)(gcn10_gpu_ctx *, void *, const void *, size_t, gcn10_stream_t);
    int (*memcpy_d2h)(gcn10_gpu_ctx *, void *, const void *, size_t, gcn10_stream_t);
    int (*memset)(gcn10_gpu_ctx *, void *, int, size_t, gcn10_stream_t);
    int (*stream_create)(gcn10_gpu_ctx *, gcn10_stream_t *);
    int (*stream_destroy)(gcn10_gpu_ctx *, gcn10_stream_t);
    int (*stream_sync)(gcn10_gpu_ctx *, gcn10_stream_t);
    int (*device_sync)(gcn10_gpu_ctx *);
    int (*event_create)(gcn10_gpu_ctx *, gcn10_event_t *);
    int (*event_destroy)(gcn10_gpu_ctx *, gcn10_event_t);
    int (*event_record)(gcn10_gpu_ctx *, gcn10_event_t, gcn10_stream_t);
    int (*event_sync)(gcn10_gpu_ctx *, gcn10_event_t);
    int (*stream_wait_event)(gcn10_gpu_ctx *, gcn10_stream_t, gcn10_event_t);
    int (*event_elapsed_ms)(gcn10_gpu_ctx *, gcn10_event_t, gcn10_event_t, float *);
    int (*set_tables)(gcn10_gpu_ctx *, const int *, int);
    int (*prepare_tile)(gcn10_gpu_ctx *, const uint8_t *, int, int, const int32_t *, int,
                        gcn10_stream_t);
    int (*cn_strip)(gcn10_gpu_ctx *, const uint8_t *, int, int, const int32_t *, unsigned, unsigned,
                    uint8_t *const[GCN10_N_RASTERS], gcn10_stream_t);
    int (*pci_bus_id)(int, char *, size_t);
    int (*inflate_tiles)(gcn10_gpu_ctx *, const uint8_t *, const gcn10_inflate_tile *, int, uint32_t, uint8_t *,
                         size_t, uint32_t *, gcn10_stream_t);
    int (*deflate_fused_available)(gcn10_gpu_ctx *);
    int (*deflate_fused_strip)(gcn10_gpu_ctx *, const uint8_t *, int, int, const int32_t *, unsigned, unsigned,
                               uint8_t *, size_t, uint32_t *, unsigned long long *, gcn10_stream_t);
    size_t (*deflate_arena_bound)(int, int, int);
    int (*deflate_strip)(gcn10_gpu_ctx *, const uint8_t *const *, int, int, int, uint8_t *, size_t,
                         uint32_t *, unsigned long long *, gcn10_stream_t);
    int (*set_option)(gcn10_gpu_ctx *, const char *, int);     /* optional (tuning): NULL when the library has none */
    size_t (*lzw_arena_bound)(int, int, int);                   /* optional: NULL when the library has none */
    int (*lzw_strip)(gcn10_gpu_ctx *, const uint8_t *const *, int, int, int, uint8_t *, size_t,
                     uint32_t *, unsigned long long *, gcn10_stream_t);
    int (*inflate_codecs)(void);    /* optional: NULL = DEFLATE and raw chunks only (LZW windows stay on the host) */
    /* optional: NULL when the library has none (needed by cog=1 only) */
    int (*overview_nearest)(gcn10_gpu_ctx *, const uint8_t *, int, int, int, uint8_t *, gcn10_stream_t);
    int (*overview_average)(gcn10_gpu_ctx *, const uint8_t *, int, int, int, int, const int32_t *, unsigned, unsigned,
                            int, uint8_t *const *, gcn10_stream_t);
    /* optional: NULL when the library has none (needed by stats=1 only) */
    int (*pair_histogram)(gcn10_gpu_ctx *, const uint8_t *, int, int, const int32_t *, unsigned long long *,
                          gcn10_stream_t);
    int (*pair_histogram_codes)(uint8_t *);
    /* optional: NULL when the library has none (needed by verify=1 only) */
    int (*verify_strip)(gcn10_gpu_ctx *, const uint8_t *, int, int, const int32_t *, unsigned, unsigned,
                        const uint8_t *const[GCN10_N_RASTERS], size_t, int, gcn10_verify_count *, gcn10_stream_t);
    int (*verify_buffers)(gcn10_gpu_ctx *, const uint8_t *const[GCN10_N_RASTERS], size_t,
                          const uint8_t *const[GCN10_N_RASTERS], size_t, int, int, int, unsigned, gcn10_verify_count *,
                          gcn10_stream_t);
    /* optional: NULL when the library has none (needed by zonal=1 only) */
    int (*zonal_pair_histogram)(gcn10_gpu_ctx *, const uint8_t *, int, int, const int32_t *, const gcn10_zone_span *,
                                const gcn10_zone_item *, size_t, int, unsigned long long *, gcn10_stream_t);
    /* optional: NULL when the library has none (needed by aggregate=<f> only) */
    int (*aggregate)(gcn10_gpu_ctx *, const uint8_t *, int, int, const int32_t *, int, int, int, unsigned, unsigned,
                     uint8_t *const *, size_t, gcn10_stream_t);
    /* optional: NULL when the library has none (needed by grid=... only) */
    int (*grid_sums)(gcn10_gpu_ctx *, const uint8_t *, int, int, const int32_t *, const int32_t *, const int32_t *, int,
                     int, unsigned, unsigned, unsigned long long *, gcn10_stream_t);
    int (*grid_finish)(gcn10_gpu_ctx *, const unsigned long long *, int, size_t, uint8_t *, const uint32_t *, uint32_t,
                       unsigned long long *, gcn10_stream_t);
    /* optional: NULL when the library has none (needed by storm=... with grid=... only) */
    int (*set_weights)(gcn10_gpu_ctx *, const uint16_t *);
    int (*grid_sums_weighted)(gcn10_gpu_ctx *, const uint8_t *, int, int, const int32_t *, const int32_t *,
                              const int32_t *, int, int, unsigned, unsigned, unsigned long long *, gcn10_stream_t);
    int (*grid_finish_weighted)(gcn10_gpu_ctx *, const unsigned long long *, int, size_t, uint8_t *, uint8_t *,
                                const uint32_t *, uint32_t, unsigned long long *, gcn10_stream_t);
    /* optional: NULL when the library has none (needed by storms=... with grid=... only) */
    int (*set_weight_tables)(gcn10_gpu_ctx *, const uint16_t *, int);
    int (*grid_sums_storms)(gcn10_gpu_ctx *, const uint8_t *, int, int, const int32_t *, const int32_t *,
                            const int32_t *, int, int, unsigned, unsigned, unsigned long long *, gcn10_stream_t);
    int (*grid_finish_storms)(gcn10_gpu_ctx *, const unsigned long long *, int, size_t, uint8_t *, uint8_t *,
                              const uint32_t *, uint32_t, unsigned long long *, gcn10_stream_t);
    /* optional: NULL when the library has none (needed by rain=... only) */
    int (*set_rain_tables)(gcn10_gpu_ctx *, const uint16_t *, int);
    int (*grid_sums_rain)(gcn10_gpu_ctx *, const uint8_t *, int, int, const int32_t *, const int32_t *, const int32_t *,
                          int, int, unsigned, unsigned, const uint8_t *, unsigned long long *, gcn10_stream_t);
    int (*grid_finish_rain)(gcn10_gpu_ctx *, const unsigned long long *, int, size_t, const uint8_t *, uint8_t *,
                            uint8_t *, const uint32_t *, uint32_t, unsigned long long *, gcn10_stream_t);
    /* optional: NULL when the library has none (needed by rains=... only, with set_rain_tables) */
    int (*grid_sums_rains)(gcn10_gpu_ctx *, const uint8_t *, int, int, const int32_t *, const int32_t *, const int32_t *,
                           int, int, unsigned, unsigned, const uint8_t *, int, unsigned long long *, gcn10_stream_t);
    int (*grid_finish_rains)(gcn10_gpu_ctx *, const unsigned long long *, int, size_t, const uint8_t *, int, uint8_t *,
                             uint8_t *, const uint32_t *, uint32_t, unsigned long long *, gcn10_stream_t);
    /* optional: NULL when the library has none (needed by zone_rain=... only) */
    int (*zonal_sums_rain)(gcn10_gpu_ctx *, const uint8_t *, int, int, const int32_t *, const gcn10_zone_span *,
                           const gcn10_zone_rain_item *, size_t, int, unsigned, unsigned, unsigned long long *,
                           gcn10_stream_t);
    /* optional: NULL when the library has none (needed by zone_rains=... only, with set_rain_tables) */
    int (*zonal_sums_rains)(gcn10_gpu_ctx *, const uint8_t *, int, int, const int32_t *, const gcn10_zone_span *,
                            const gcn10_zone_rains_item *, size_t, int, unsigned, unsigned, int, unsigned long long *,
                            gcn10_stream_t);
    /* optional: NULL when the library has none (needed by runoff_rain=... only) */
    int (*set_cell_byte_tables)(gcn10_gpu_ctx *, const uint8_t *, int);
    int (*runoff_strip)(gcn10_gpu_ctx *, const uint8_t *, int, int, const int32_t *, const int32_t *, const int32_t *, int,
                        int, const uint8_t *, unsigned, unsigned, uint8_t *const[GCN10_N_RASTERS], gcn10_stream_t);
};
const struct gcn10_gpu_api *gcn10_gpu_api_get(char *err, size_t errcap);


#endif
