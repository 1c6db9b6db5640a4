/*
 * gcn10_gpu.h -- C ABI of the MI355X (gfx950) curve-number engine.
 *
 * This is the drop-in boundary for gcn10's per-pixel path.  The reference has
 * no FFI layer; its seam is the set of C prototypes in src/global.h:47-71 and
 * the static kernels of src/cn.c.  Each entry point below names the reference
 * code it replaces.  Plain C types only: no HIP or torch types cross this line.
 * A stream or event is an opaque pointer (a hipStream_t / hipEvent_t inside);
 * passing NULL as a stream means "the context's own main stream".
 *
 * All functions returning int give 0 on success or a negative GCN10_E_* code;
 * gcn10_gpu_last_error() returns the calling thread's last message.  The
 * reference's functions are void and log-then-return or MPI_Abort
 * (src/cn.c:156-160, 25); the host driver maps these codes back to that
 * behaviour.
 *
 * Threading: a context belongs to one GPU and is used by one host thread at a
 * time (the reference runs one thread per rank, src/main.c:171-176).  The one
 * exception: gcn10_gpu_event_sync() only reads the context and may be called by
 * other threads while its owner works (the host pipeline's I/O threads wait for
 * a strip's copy-back that way).
 *
 * There is no CPU fallback behind this ABI: every call needs a live gfx950
 * device, and gcn10_gpu_init() fails loudly without one.
 */
#ifndef GCN10_GPU_H
#define GCN10_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1: round 1.  2: + gcn10_gpu_tune_single_raster, gcn10_gpu_stream_copy, gcn10_gpu_soil_words_state (round 2).
 * 3: gcn10_inflate_tile.reserved became .flags (raw and predictor-2 chunks), the tile encoders lay a raster's
 *    streams of a strip out as one extent (option "arena_segment_align"), gcn10_gpu_deflate_arena_bound grew by
 *    the extents' pads (round 3).  A caller built against an older header must be rebuilt: check at start-up.
 *    Added within 3: the LZW encoder (gcn10_gpu_lzw_*), LZW tiles of gcn10_gpu_inflate_tiles (GCN10_TILE_LZW)
 *    and gcn10_gpu_inflate_codecs; the overview kernels of the COG output (gcn10_gpu_overview_*); the pair histogram
 *    of the band statistics (gcn10_gpu_pair_histogram*); the raster verifier (gcn10_gpu_verify_*); the pair histogram
 *    per zone of the zonal composites (gcn10_gpu_zonal_pair_histogram); the area means on a coarser grid
 *    (gcn10_gpu_aggregate); the sums and means on a model grid (gcn10_gpu_grid_sums, gcn10_gpu_grid_finish) and their
 *    weighted forms (gcn10_gpu_set_weights, gcn10_gpu_grid_sums_weighted, gcn10_gpu_grid_finish_weighted), and those
 *    for several weight tables (gcn10_gpu_set_weight_tables, gcn10_gpu_grid_sums_storms, gcn10_gpu_grid_finish_storms);
 *    the sums with a weight table per cell (gcn10_gpu_set_rain_tables, gcn10_gpu_grid_sums_rain,
 *    gcn10_gpu_grid_finish_rain, gcn10_gpu_grid_rain_item); the sums per zone with a weight table per piece of a zone
 *    (gcn10_gpu_zonal_sums_rain); the sums with several weight tables per cell (gcn10_gpu_grid_sums_rains,
 *    gcn10_gpu_grid_finish_rains); the rasters of a strip through a byte table per cell
 *    (gcn10_gpu_set_cell_byte_tables, gcn10_gpu_runoff_strip).
 *    Removed within 3: the four timing-experiment options of gcn10_gpu_set_option (round 3); they are unknown names now. */
#define GCN10_GPU_ABI_VERSION 3

enum {
    GCN10_OK = 0,
    GCN10_E_INVAL = -1,     /* bad argument (null pointer, size, mask)        */
    GCN10_E_HIP = -2,       /* a HIP runtime call failed; see last_error      */
    GCN10_E_NOMEM = -3,     /* device or pinned-host allocation failed        */
    GCN10_E_STATE = -4,     /* call order: tables / tile not prepared         */
    GCN10_E_NODEVICE = -5   /* no gfx950 device visible                       */
};

/* Raster order of the 18 outputs of one block: index = cond*9 + hc*3 + arc,
 * cond in {drained, undrained}, hc in {p, f, g}, arc in {i, ii, iii}
 * -- the loop order of src/cn.c:145-147, 236-259. */
#define GCN10_N_TABLES 9
#define GCN10_N_CONDS 2
#define GCN10_N_RASTERS 18
#define GCN10_COND_DRAINED 1u       /* cond_mask bit for conds[0] (src/cn.c:145) */
#define GCN10_COND_UNDRAINED 2u     /* cond_mask bit for conds[1]                */
#define GCN10_NODATA 255            /* src/cn.c:38, 289                          */

typedef struct gcn10_gpu_ctx gcn10_gpu_ctx;
typedef void *gcn10_stream_t;
typedef void *gcn10_event_t;

/* ---- life cycle -------------------------------------------------------- */

int gcn10_gpu_abi_version(void);
/* Number of visible HIP devices (0 when there is none or the runtime fails). */
int gcn10_gpu_device_count(void);
/* One context per GPU.  Replaces the per-rank process state of the reference
 * (MPI_Init + rank, src/main.c:80-82): "rank" becomes the device index. */
int gcn10_gpu_init(int device, gcn10_gpu_ctx **ctx);
void gcn10_gpu_destroy(gcn10_gpu_ctx *ctx);
const char *gcn10_gpu_last_error(void);
/* Fills name[cap] with the device name and returns CU count, or <0. */
int gcn10_gpu_device_info(gcn10_gpu_ctx *ctx, char *name, size_t cap,
                          size_t *hbm_bytes);

/* PCI address of HIP device `device` as "dddd:bb:dd.f" (for NUMA placement of the
 * host thread that feeds it); works without a context.  0 or <0. */
int gcn10_gpu_pci_bus_id(int device, char *buf, size_t cap);

/* ---- memory, streams, events ------------------------------------------ */
/* The reference mallocs every raster on the host (src/raster.c:169,
 * src/cn.c:209,264,278).  Here rasters live in HBM; the host stages them
 * through pinned buffers (replaces GDALRasterIO's destination buffer,
 * src/raster.c:176-178, 217-219). */

int gcn10_gpu_malloc(gcn10_gpu_ctx *ctx, size_t bytes, void **dptr);
int gcn10_gpu_free(gcn10_gpu_ctx *ctx, void *dptr);
int gcn10_gpu_host_alloc(gcn10_gpu_ctx *ctx, size_t bytes, void **hptr);
int gcn10_gpu_host_free(gcn10_gpu_ctx *ctx, void *hptr);
/* Asynchronous on `stream`; the host buffer must be pinned for real overlap. */
int gcn10_gpu_memcpy_h2d(gcn10_gpu_ctx *ctx, void *dst_dev, const void *src_host,
                         size_t bytes, gcn10_stream_t stream);
int gcn10_gpu_memcpy_d2h(gcn10_gpu_ctx *ctx, void *dst_host, const void *src_dev,
                         size_t bytes, gcn10_stream_t stream);
int gcn10_gpu_memset(gcn10_gpu_ctx *ctx, void *dptr, int value, size_t bytes,
                     gcn10_stream_t stream);

int gcn10_gpu_stream_create(gcn10_gpu_ctx *ctx, gcn10_stream_t *stream);
int gcn10_gpu_stream_destroy(gcn10_gpu_ctx *ctx, gcn10_stream_t stream);
int gcn10_gpu_stream_sync(gcn10_gpu_ctx *ctx, gcn10_stream_t stream);
int gcn10_gpu_device_sync(gcn10_gpu_ctx *ctx);
int gcn10_gpu_event_create(gcn10_gpu_ctx *ctx, gcn10_event_t *ev);
int gcn10_gpu_event_destroy(gcn10_gpu_ctx *ctx, gcn10_event_t ev);
int gcn10_gpu_event_record(gcn10_gpu_ctx *ctx, gcn10_event_t ev, gcn10_stream_t stream);
int gcn10_gpu_event_sync(gcn10_gpu_ctx *ctx, gcn10_event_t ev);
/* Makes `stream` wait for `ev` (device-side; the host does not block). */
int gcn10_gpu_stream_wait_event(gcn10_gpu_ctx *ctx, gcn10_stream_t stream, gcn10_event_t ev);
int gcn10_gpu_event_elapsed_ms(gcn10_gpu_ctx *ctx, gcn10_event_t start,
                               gcn10_event_t stop, float *ms);

/* ---- lookup tables ----------------------------------------------------- */
/* Replaces the hand-off `int table[256][5]` from load_lookup_table() to
 * calculate_cn() (src/cn.c:148, 261, 290).  `tables` is n_tables consecutive
 * reference-format tables, i.e. int[n_tables][256][5] exactly as
 * load_lookup_table fills them (255 = nodata).  The engine folds the
 * `cn_value < 255 ? (uint8_t)cn_value : keep 255` rule of src/cn.c:125-128
 * into byte tables once, and keeps them on the device until replaced.
 * 1 <= n_tables <= 9. */
int gcn10_gpu_set_tables(gcn10_gpu_ctx *ctx, const int *tables, int n_tables);

/* ---- per-function kernels (one reference function each) ---------------- */

/* src/cn.c:218-232, the resample loop, with its separable index arithmetic
 * hoisted to the host: ci[W] and cj[rows] are the clamped coarse column / row
 * of every fine column / row (gcn10_build_index_maps in gcn10_host.h computes
 * them in the reference's exact fp64 order).  out[y*W+x] =
 * coarse[cj[y]*hsx+ci[x]].  All pointers are device pointers. */
int gcn10_gpu_resample(gcn10_gpu_ctx *ctx, const uint8_t *coarse, int hsx, int hsy,
                       const int32_t *ci, const int32_t *cj, int W, int rows,
                       uint8_t *out, gcn10_stream_t stream);

/* src/cn.c:88-111 modify_hysogs_data(), in place on a device buffer;
 * drained != 0 <=> cond == "drained". */
int gcn10_gpu_modify_hysogs_data(gcn10_gpu_ctx *ctx, uint8_t *h, size_t npix,
                                 int drained, gcn10_stream_t stream);

/* src/cn.c:114-131 calculate_cn() on a raster the reference pre-fills with 255
 * (src/cn.c:289): out[i] = (hsg[i] < 5 && T[esa[i]][hsg[i]] < 255) ?
 * (uint8_t)T[esa[i]][hsg[i]] : 255, T = table `table_index` of set_tables. */
int gcn10_gpu_calculate_cn(gcn10_gpu_ctx *ctx, const uint8_t *esa,
                           const uint8_t *hsg, size_t npix, int table_index,
                           uint8_t *out, gcn10_stream_t stream);

/* ---- fused block path --------------------------------------------------- */
/* Replaces the body of process_block() between load_raster and save_raster
 * (src/cn.c:205-290): resample + memcpy + modify_hysogs_data + memset +
 * calculate_cn for every (cond, hc, arc), in one pass over the landcover.
 *
 * gcn10_gpu_prepare_tile: once per block.  Takes a snapshot of the soil of
 * the block into memory owned by the context -- the x half of
 * src/cn.c:218-232: the soil code of every coarse cell (hsx * hsy bytes) and
 * the clamped coarse column of every fine column (ci[x] < 0 or >= hsx names
 * column hsx - 1); it also notes whether every 16-pixel column group of the
 * tile is compact, i.e. a run of one coarse column followed by a run of
 * another.  Nothing is written per coarse row and column group.  `coarse`
 * and `ci` are not read after the kernel this call launches: the caller may
 * reuse them once `stream` has passed it.
 * Strips whose width is a multiple of 16 read that snapshot directly: every
 * lane of the strip kernel stays in one column group for the whole launch,
 * makes the group's two coarse columns and the position where the second
 * begins from the column map once, and loads the two cell codes of its
 * coarse row per 16 pixels.  When some group of the tile is not compact they
 * take the code of every pixel from the cell codes through the column map
 * (gcn10_gpu_soil_words_state).  Everything else that needs soil -- strips of
 * other widths or of unaligned rasters, strips with "compact_soil" off,
 * strips with more column groups in a row than the launch has threads, the
 * fused encoder, verify, the pair histograms, the average overviews, the
 * area means of gcn10_gpu_aggregate -- reads one code byte per fine column
 * and coarse row from a workspace (hsy rows of W bytes) that is allocated here and filled from the tables by the first
 * such call after prepare_tile, on that call's stream; a later reader on
 * another stream waits for that through an event of the context.  The order
 * the caller has to provide is the one below and no other: every reader's
 * stream is ordered after prepare_tile's, and the next prepare_tile after the
 * readers of this one.
 *
 * gcn10_gpu_cn_strip: any number of times per block, one row strip each
 * (rows y0 .. y0+rows of the block; `esa` and every out[] pointer address the
 * first pixel of the strip; cj points at the strip's first entry, i.e.
 * &cj_block[y0]).  For every selected raster r = cond*9 + k it writes
 *     h = coarse[cj[y]*hsx + ci[x]];  s = remap_cond(h)   (src/cn.c:88-111)
 *     out[r][y*W+x] = s < 5 ? T8[k][esa[y*W+x]][s] : 255  (src/cn.c:114-131)
 * cond_mask: GCN10_COND_* bits; table_mask: bit k selects table k (< n_tables).
 * out[] has GCN10_N_RASTERS entries (host array of device pointers); entries
 * of unselected rasters are ignored and may be NULL.  Strips of one block may
 * be issued on different streams once prepare_tile's stream work is ordered
 * before them (event or sync).
 * out[] must point into ordinary device allocations (gcn10_gpu_malloc / hipMalloc).
 * Ranges assembled with HIP's virtual memory management (hipMemCreate + hipMemMap)
 * are not supported: the kernels store nontemporally, and such stores into chunk-
 * mapped ranges were observed not to be visible yet when the kernel had completed
 * (ROCm 7.2, MI355X; profiles/r02/spread_allocator_hazard.txt). */
int gcn10_gpu_prepare_tile(gcn10_gpu_ctx *ctx, const uint8_t *coarse, int hsx,
                           int hsy, const int32_t *ci, int W,
                           gcn10_stream_t stream);
int gcn10_gpu_cn_strip(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows,
                       const int32_t *cj, unsigned cond_mask, unsigned table_mask,
                       uint8_t *const out[GCN10_N_RASTERS], gcn10_stream_t stream);

/* Bytes the dominant kernel (cn_strip) must move per launch by the algorithm:
 * W*rows*(1 + n_selected_rasters) + the x-expanded soil rows it reads once.
 * Used by the benchmark for the roofline figure ("algorithmic
 * bytes"). */
size_t gcn10_gpu_strip_algorithmic_bytes(int W, int rows, int hsx, int hsy,
                                         unsigned cond_mask, unsigned table_mask);

/* ---- output encode: the DEFLATE of save_raster(), on the GPU --------------- */
/* Replaces the zlib work inside save_raster()'s GDALRasterIO (src/raster.c:204-219:
 * GTiff, COMPRESS=DEFLATE, TILED=YES, i.e. one zlib stream per 256x256 block).
 * Every 256x256 tile of `n_rasters` device raster strips (W x rows each, row
 * major; edge tiles zero padded) becomes one complete zlib stream (RFC 1950/1951,
 * dynamic Huffman) in `arena_dev`; table_dev[(r*tiles + ty*across + tx)*2 + {0,1}]
 * receives the stream's byte offset in the arena and its size (offset 0xffffffff:
 * the arena was too small); *cursor_dev receives the number of arena bytes used.
 * The arena: streams lie in index order (raster-major, tiles row-major), each in a slot of
 * its size rounded up to 16 bytes; raster 0's extent starts at 0, every later raster's at
 * the next multiple of "arena_segment_align" (gcn10_gpu_set_option) behind the previous
 * raster's last slot; the cursor is the end of the last raster's last slot, not aligned.
 * A stream fits iff offset + slot <= arena_cap.  Inside [0, ceil_align(cursor)) every byte
 * is part of a stream or ZERO -- slot tails, the pads between extents and the pad behind
 * the last one are written as zeros, in whole 16-byte units that end at or before
 * arena_cap -- because the host writes whole extents into the files; no other byte of the
 * arena, and none at or behind arena_cap, is touched (tests/arena_model.py states the
 * rule in Python; tests/test_gpu_arena.py holds all three encoders to it).
 * rasters_dev is a DEVICE array of n_rasters device pointers.  Asynchronous on
 * `stream`.  The raw rasters never have to cross PCIe. */
size_t gcn10_gpu_deflate_arena_bound(int W, int rows, int n_rasters);
int gcn10_gpu_deflate_strip(gcn10_gpu_ctx *ctx, const uint8_t *const *rasters_dev,
                            int n_rasters, int W, int rows, uint8_t *arena_dev,
                            size_t arena_cap, uint32_t *table_dev,
                            unsigned long long *cursor_dev, gcn10_stream_t stream);

/* The same contract with TIFF LZW streams (TIFF 6.0 section 13, Compression 5; config key compress=lzw): every
 * 256x256 tile (edge tiles zero padded) becomes one complete LZW stream -- MSB-first 9..12-bit codes, early
 * change, starting with ClearCode, ending with EndOfInformation, padded to a byte -- and streams, table and
 * cursor are laid out exactly as by gcn10_gpu_deflate_strip (offset 0xffffffff: the arena was too small; nothing
 * is written past arena_cap).  gcn10_gpu_lzw_arena_bound covers incompressible tiles.  Added in ABI 3 without a
 * version change: a caller that needs them looks them up (the host program does, and only for LZW runs). */
size_t gcn10_gpu_lzw_arena_bound(int W, int rows, int n_rasters);
int gcn10_gpu_lzw_strip(gcn10_gpu_ctx *ctx, const uint8_t *const *rasters_dev, int n_rasters, int W, int rows,
                        uint8_t *arena_dev, size_t arena_cap, uint32_t *table_dev,
                        unsigned long long *cursor_dev, gcn10_stream_t stream);

/* The same encoding WITHOUT materialising the CN rasters: the strip's landcover and the
 * block's x-expanded soil (gcn10_gpu_prepare_tile) are reduced to pixel classes once per
 * tile position, tokenised once, and the selected rasters' streams are produced from that
 * (src/cn.c:236-290 and the zlib of src/raster.c:204-219 in one device pass; no CN raster
 * is written to or read from HBM).  Stream r' of the table is the r'-th selected raster in
 * ascending raster order (cond*9 + hc*3 + arc).  Needs the tables to define at most 256
 * distinct 18-vectors (GCN10_E_STATE otherwise; the shipped tables define about 110).
 * Two table entries may name the same arena bytes: where no dual soil class lies under a tile,
 * the drained and the undrained raster of a table are the same stream, emitted once. */
int gcn10_gpu_deflate_fused_available(gcn10_gpu_ctx *ctx);     /* 1 after set_tables if <= 256 classes */
int gcn10_gpu_deflate_fused_strip(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows,
                                  const int32_t *cj, unsigned cond_mask, unsigned table_mask,
                                  uint8_t *arena_dev, size_t arena_cap, uint32_t *table_dev,
                                  unsigned long long *cursor_dev, gcn10_stream_t stream);

/* Landcover input decode on the GPU (replaces the inflate GDALRasterIO does on the host inside
 * load_raster, /root/reference/src/raster.c:167-176).  `tiles_dev` describes n_tiles zlib
 * streams (TIFF Compression 8 / 32946: one per tile or strip of the landcover files) lying in
 * `comp_dev`; every stream is decoded by one workgroup (a decoder and a copier wavefront) into
 * a linear slot of at most chunk_bytes, and the wanted window of each chunk (copy_w x copy_h pixels from (src_x, src_y)
 * of a chunk chunk_w pixels wide) is copied to dst_dev + dst_off, rows dst_stride apart.
 * status_dev[i] = 0, or the reason stream i is not a valid zlib stream (GCN10_INFLATE_E_*); a
 * stream that ends early leaves zeros, one that is longer than out_len is cut there, as the
 * host reader (tiff_codec.c) does.  Streams must start at multiples of 16 bytes in comp_dev, and
 * comp_dev must be readable up to the next multiple of 4 past every stream's end. */
typedef struct gcn10_inflate_tile {
    uint64_t in_off;        /* byte offset of the zlib stream in comp_dev, multiple of 16 */
    uint32_t in_len;        /* its size in bytes */
    uint32_t out_len;       /* bytes the chunk decodes to: chunk_w * rows in the chunk */
    uint32_t chunk_w;       /* pixels per row of the decoded chunk */
    uint32_t src_x, src_y;  /* first wanted pixel of the chunk */
    uint32_t copy_w, copy_h;
    uint32_t flags;         /* GCN10_TILE_* (ABI 3; 0 = a zlib stream, no predictor, as in ABI 1-2) */
    uint64_t dst_off;       /* where pixel (src_x, src_y) goes in dst_dev */
} gcn10_inflate_tile;
/* flags: RAW = the chunk is not compressed (TIFF Compression 1): in_len >= out_len bytes of pixels lie at
 * in_off and only the window copy is done (no alignment rule for in_off; the host may stage only the bytes
 * from the first wanted pixel on: src_x = src_y = 0 then, chunk_w still the chunk's row pitch).
 * PREDICTOR2 = the chunk was written with TIFF Predictor 2 (horizontal differencing): every chunk row is
 * summed back, byte-wise modulo 256, from the row's first pixel while it is copied (tiff_codec.c gcn10_tiff_decode_chunk does
 * the same on the host).
 * LZW = the chunk is a TIFF LZW stream (Compression 5: MSB-first codes, early change), decoded as tiff_codec.c
 * lzw_decode does (an early EOI leaves zeros, codes past out_len are ignored); same alignment rule as a zlib
 * stream.  May be combined with PREDICTOR2, not with RAW (status GCN10_INFLATE_E_HEADER).  One call may mix
 * zlib, raw and LZW tiles. */
#define GCN10_TILE_RAW 1u
#define GCN10_TILE_PREDICTOR2 2u
#define GCN10_TILE_LZW 4u
enum {
    GCN10_INFLATE_E_HEADER = 1, GCN10_INFLATE_E_BLOCK_TYPE = 2, GCN10_INFLATE_E_STORED = 3,
    GCN10_INFLATE_E_LENGTHS = 4, GCN10_INFLATE_E_CODE = 5, GCN10_INFLATE_E_DISTANCE = 6,
    GCN10_INFLATE_E_INPUT = 7, GCN10_INFLATE_E_WINDOW = 8,
    /* LZW tiles: a code beyond the dictionary (code > next); the first code of the stream or after a
     * ClearCode is not a literal; the input ends without EndOfInformation before out_len bytes */
    GCN10_INFLATE_E_LZW_CODE = 9, GCN10_INFLATE_E_LZW_FIRST = 10, GCN10_INFLATE_E_LZW_INPUT = 11
};
int gcn10_gpu_inflate_tiles(gcn10_gpu_ctx *ctx, const uint8_t *comp_dev,
                            const gcn10_inflate_tile *tiles_dev, int n_tiles, uint32_t chunk_bytes,
                            uint8_t *dst_dev, size_t dst_stride, uint32_t *status_dev,
                            gcn10_stream_t stream);
/* The chunk codecs gcn10_gpu_inflate_tiles decodes, GCN10_CODEC_* bits (a library without this symbol
 * decodes DEFLATE and raw chunks only). */
#define GCN10_CODEC_DEFLATE 1u
#define GCN10_CODEC_RAW 2u
#define GCN10_CODEC_LZW 4u
int gcn10_gpu_inflate_codecs(void);

/* Overviews of the Cloud Optimized GeoTIFF output (config key cog=1).  Level k of a W x H block is
 * ceil(W / 2^k) x ceil(H / 2^k).  Added in ABI 3 without a version change; the host looks them up for cog runs only.
 *
 * gcn10_gpu_overview_nearest: dst (level k, row major) = src (W x H landcover, row major) sampled at
 *   (min(2^k x + 2^(k-1), W-1), min(2^k y + 2^(k-1), H-1)), 1 <= level.  Such a level is a block of its own for
 *   gcn10_gpu_prepare_tile and the strip encoders (its soil index maps are the block's, composed the same way).
 * gcn10_gpu_overview_average: levels 1 .. n_levels (1..8) of every selected raster for the full-resolution rows
 *   [y0, y0 + rows) of a block, straight from its landcover (`esa`: the block's row 0, `cj`: the block's soil rows)
 *   and the soil gcn10_gpu_prepare_tile prepared for width W: no full-resolution CN raster is made.  Level k pixel =
 *   the clipped 2x2 footprint in level k-1 (level 0 = the CN raster src/cn.c:114-131 defines) without the value 255,
 *   (2 s + n) / (2 n) in integers, 255 when n = 0.  y0 and rows are multiples of 256 (rows may end at H), so a strip
 *   gives whole rows of every level.  levels: host array of n_selected * n_levels device pointers, [q * n_levels +
 *   k - 1] = level k of the q-th selected raster in ascending raster order, each a whole level raster (the call
 *   writes the strip's rows of it). */
int gcn10_gpu_overview_nearest(gcn10_gpu_ctx *ctx, const uint8_t *src, int W, int H, int level, uint8_t *dst,
                               gcn10_stream_t stream);
int gcn10_gpu_overview_average(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int H, int y0, int rows,
                               const int32_t *cj, unsigned cond_mask, unsigned table_mask, int n_levels,
                               uint8_t *const *levels, gcn10_stream_t stream);

/* Band statistics of the outputs (config key stats=1).  Every raster's value at a pixel is a function of the pixel's
 * (landcover byte, soil code byte) pair -- soil code = drained plane | undrained plane << 4, as the strip kernels
 * derive it from the soil class (src/cn.c:88-111) --, so one histogram of those pairs per block gives the exact
 * histogram of all 18 rasters on the host (gcn10_raster_histogram in gcn10_host.h).  The codes are kept in
 * GCN10_PAIR_HIST_BINS dense bins: hist[bin * 256 + landcover].  Added in ABI 3 without a version change; the host
 * looks them up for stats runs only.
 *
 * gcn10_gpu_pair_histogram_codes: codes[b] = the soil code counted in bin b (bins no code maps to hold 0x55, the
 *   invalid plane in both conditions, and stay empty).  Returns GCN10_PAIR_HIST_BINS.
 * gcn10_gpu_pair_histogram: ADDS the pair counts of one strip (`esa`: W x rows landcover, row major; `cj`: the soil
 *   row of each of its rows, as for gcn10_gpu_cn_strip) to the device histogram hist_dev[GCN10_PAIR_HIST_SIZE], with
 *   the soil codes gcn10_gpu_prepare_tile prepared for width W.  Only the W x rows pixels are counted (no tile
 *   padding); 64-bit counters.  Asynchronous on `stream`; clear hist_dev once per block (gcn10_gpu_memset). */
#define GCN10_PAIR_HIST_BINS 16
#define GCN10_PAIR_HIST_SIZE (256 * GCN10_PAIR_HIST_BINS)
int gcn10_gpu_pair_histogram_codes(uint8_t codes[GCN10_PAIR_HIST_BINS]);
int gcn10_gpu_pair_histogram(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                             unsigned long long *hist_dev, gcn10_stream_t stream);

/* Composite curve numbers per zone (config key zonal=1): the same pair counts restricted to the pixels of zones.  Added
 * in ABI 3 without a version change; the host looks it up for zonal runs only.
 *
 * gcn10_gpu_zonal_pair_histogram: ADDS to hist_dev[zone * GCN10_PAIR_HIST_SIZE + bin * 256 + landcover] the pair counts
 *   of the pixels of every span -- columns [x0, x1) of row y, y relative to esa's first row.  esa, W, rows, cj, the
 *   soil prepared by gcn10_gpu_prepare_tile, the bin layout and the 64-bit counters are exactly those of
 *   gcn10_gpu_pair_histogram.  spans_dev is sorted by zone; items_dev[i] names n_spans consecutive spans of ONE zone
 *   from first_span on, and together the items name every span once (gcn10_zones_build_plan / gcn10_zone_items_build
 *   of gcn10_host.h make both; a workgroup takes a contiguous run of items).  The caller guarantees 0 <= y < rows,
 *   0 <= x0 < x1 <= W and 0 <= zone < n_zones: the kernel does not check them.  n_items == 0 is a successful no-op.
 *   Asynchronous on `stream`; clear hist_dev once (gcn10_gpu_memset).  Pixels named by two spans count twice.  A workgroup
 *   counts a zone in 32-bit words until the zone changes, so the spans of one zone in one call name fewer than 2^32
 *   pixels in all (a block has at most 2^31, and the builder names each once). */
#ifndef GCN10_ZONE_SPAN_DEFINED
#define GCN10_ZONE_SPAN_DEFINED
typedef struct gcn10_zone_span { int32_t y, x0, x1, zone; } gcn10_zone_span;       /* columns [x0, x1) of row y */
typedef struct gcn10_zone_item { uint32_t first_span, n_spans; } gcn10_zone_item;
#endif
int gcn10_gpu_zonal_pair_histogram(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                                   const gcn10_zone_span *spans_dev, const gcn10_zone_item *items_dev, size_t n_items,
                                   int n_zones, unsigned long long *hist_dev /* [n_zones][GCN10_PAIR_HIST_SIZE] */,
                                   gcn10_stream_t stream);

/* Area-mean rasters on a coarser grid (config key aggregate=<f>).  Added in ABI 3 without a version change; the host
 * looks it up for aggregate runs only.
 *
 * gcn10_gpu_aggregate: `esa`, W, rows, `cj` and the soil prepared by gcn10_gpu_prepare_tile are those of
 *   gcn10_gpu_pair_histogram: `rows` landcover rows of width W, which must start at a cell-row boundary.  Cell
 *   (cx, cy) covers columns x0 + cx f .. min(x0 + (cx + 1) f, x1) - 1 and rows cy f .. min((cy + 1) f, rows) - 1.
 *   With v the value gcn10_gpu_cn_strip writes for a raster at a pixel, s the sum and n the count of the
 *   footprint's v != 255, the cell is (2 s + n) / (2 n) in integers (round half up), 255 when n = 0.  out[q] is the
 *   q-th selected raster in ascending raster order (host array of device pointers): ceil(rows / f) rows of
 *   ceil((x1 - x0) / f) bytes, out_stride bytes apart; nothing else of out is written.  The call writes whole
 *   output rows: a caller that cuts a block into bands gives every band but the last a multiple of f rows.  Calls
 *   never add to each other's cells; the bytes do not depend on the launch shape.  Any W, any alignment of esa.
 *   GCN10_E_INVAL: factor outside 2..256, x0 < 0, x0 >= x1, x1 > W, rows <= 0, out_stride < ceil((x1 - x0) / f), the
 *   masks.  Asynchronous on `stream`. */
int gcn10_gpu_aggregate(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                        int x0, int x1, int factor, unsigned cond_mask, unsigned table_mask,
                        uint8_t *const *out, size_t out_stride, gcn10_stream_t stream);

/* Mean-CN rasters on a model grid (config key grid=...).  Added in ABI 3 without a version change; the host looks them
 * up for grid runs only.
 *
 * gcn10_gpu_grid_sums: `esa`, W, rows, `cj` and the soil prepared by gcn10_gpu_prepare_tile are those of
 *   gcn10_gpu_pair_histogram.  cellx_dev[W] and celly_dev[rows] give the cell column of every pixel column and the
 *   cell row of every strip row, in 0 .. ncx - 1 and 0 .. ncy - 1, anything else (-1) meaning "in no cell"
 *   (gcn10_grid_plan_block of gcn10_host.h makes them).  Their entries that name a cell never decrease, and any 16
 *   columns from a multiple of 16 on name at most three cell columns (cells of 8 pixels or more): pixels of a fourth
 *   one are left out.  ADDS, for every selected raster q (ascending raster order) and every pixel (x, y) with
 *   cellx[x] and celly[y] naming a cell and value v != 255 -- v what gcn10_gpu_cn_strip writes for that raster at that
 *   pixel --, v to acc[q][celly[y]][cellx[x]][0] and 1 to ...[1].  Integers only: the pairs do not depend on the
 *   launch shape, on how a caller cuts the rows into calls, or on order.  Any W, any alignment of esa; nothing at or
 *   beyond W is read; nothing outside acc's n_sel * ncy * ncx pairs is written.
 * gcn10_gpu_grid_finish: means[q * n_cells + c] = n ? (2 s + n) / (2 n) : 255 (the rule of gcn10_gpu_aggregate) for
 *   the pair {s, n} = acc[q * n_cells + c] of every raster q < n_sel and cell c < n_cells, and the pairs of the
 *   n_shared cells shared_idx_dev names, packed: shared[q * n_shared + i] = acc[q * n_cells + shared_idx[i]]
 *   (shared_idx[i] < n_cells is the caller's to guarantee; n_shared == 0: both pointers may be NULL).
 * Neither reads weights: on a context that holds weight tables (below) both still work on pairs.  One sums kernel and
 *   one finish kernel serve these two calls (no table), the _weighted calls (one) and the _storms calls (k).
 * GCN10_E_INVAL: the masks, W, rows, ncx or ncy <= 0, a null pointer (grid_sums); n_sel outside 1..18, n_cells == 0 or
 *   >= 2^32, a null pointer (grid_finish).  GCN10_E_STATE: grid_sums without tables or without a tile prepared for
 *   width W, as gcn10_gpu_aggregate (grid_finish reads no tile).  Asynchronous on `stream`. */
int gcn10_gpu_grid_sums(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                        const int32_t *cellx_dev, const int32_t *celly_dev, int ncx, int ncy,
                        unsigned cond_mask, unsigned table_mask,
                        unsigned long long *acc /* [n_sel][ncy][ncx][2] = {s, n} */, gcn10_stream_t stream);
int gcn10_gpu_grid_finish(gcn10_gpu_ctx *ctx, const unsigned long long *acc, int n_sel, size_t n_cells, uint8_t *means,
                          const uint32_t *shared_idx_dev, uint32_t n_shared, unsigned long long *shared,
                          gcn10_stream_t stream);

/* Weighted sums on a model grid (config key storm=...: the runoff-weighted composites).  Added in ABI 3 without a
 * version change; the host looks them up for storm runs on a grid only.
 *
 * gcn10_gpu_set_weights: w[256], a 16-bit weight per raster value (host memory; w[255] is never read).  Called after
 *   gcn10_gpu_set_tables, with no weighted call in flight: it folds w into two images of the loaded tables (the low
 *   and the high bytes of w[value], zero where there is no value) and keeps w for gcn10_gpu_grid_finish_weighted.
 *   Synchronous.  A later gcn10_gpu_set_tables invalidates the weights: the two weighted calls then answer
 *   GCN10_E_STATE ("call gcn10_gpu_set_weights first") until it is called again.
 * gcn10_gpu_grid_sums_weighted: every word of gcn10_gpu_grid_sums -- the maps, the -1 rule, three cell columns per
 *   group of 16, ADD semantics, nothing read at or beyond W, nothing written outside acc whatever the maps hold --
 *   with triples {s, n, sw} instead of pairs: words 0 and 1 are exactly what gcn10_gpu_grid_sums adds, word 2 gets the
 *   sum of w[v] over the same pixels (v != 255).  Integers only: the triples do not depend on bands, chunks or order.
 * gcn10_gpu_grid_finish_weighted: means[] as gcn10_gpu_grid_finish writes it; cnq[q * n_cells + c] = the
 *   runoff-equivalent value of the triple by the rule of gcn10_runoff_cn (gcn10_host.h) with the context's weights:
 *   255 when n = 0, the mean byte when sw = 0, else the smallest c in 1..100 with n * w[c] >= sw (100 when there is
 *   none); and the triples of the shared cells, packed: shared[q * n_shared + i] = acc[q * n_cells + shared_idx[i]].
 * Errors as the unweighted calls', cnq among the pointers. */
int gcn10_gpu_set_weights(gcn10_gpu_ctx *ctx, const uint16_t *w /* [256] */);
int gcn10_gpu_grid_sums_weighted(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                                 const int32_t *cellx_dev, const int32_t *celly_dev, int ncx, int ncy,
                                 unsigned cond_mask, unsigned table_mask,
                                 unsigned long long *acc /* [n_sel][ncy][ncx][3] = {s, n, sw} */,
                                 gcn10_stream_t stream);
int gcn10_gpu_grid_finish_weighted(gcn10_gpu_ctx *ctx, const unsigned long long *acc, int n_sel, size_t n_cells,
                                   uint8_t *means, uint8_t *cnq, const uint32_t *shared_idx_dev, uint32_t n_shared,
                                   unsigned long long *shared, gcn10_stream_t stream);

/* Several weight tables in one pass (config key storms=...: a ladder of design storms).  Added in ABI 3 without a
 * version change, as the weighted calls were; the host looks them up for storms runs on a grid only.
 *
 * gcn10_gpu_set_weight_tables: w[k][256], 1 <= k <= GCN10_GPU_MAX_WEIGHT_TABLES tables as gcn10_gpu_set_weights takes
 *   one: every table is folded into its low and its high plane (2 k images behind each other), and the k tables and a
 *   "never decreases" flag per table are kept for the finish pass.  gcn10_gpu_set_weights(ctx, w) equals k = 1.  A
 *   later gcn10_gpu_set_tables invalidates all of it.
 * gcn10_gpu_grid_sums_storms: every word of gcn10_gpu_grid_sums_weighted with 2 + k words per (raster, cell) instead of
 *   three: words 0 and 1 are exactly what gcn10_gpu_grid_sums adds, word 2 + j gets the sum of w_j[v] over the same
 *   pixels.  With k = 1 it adds exactly what gcn10_gpu_grid_sums_weighted adds.
 * gcn10_gpu_grid_finish_storms: means[] as gcn10_gpu_grid_finish writes it; cnq[(j * n_sel + q) * n_cells + c] = the
 *   value of (s, n, word 2 + j) by the rule of gcn10_runoff_cn with table j -- bisection for a table whose entries
 *   1..100 never decrease, a scan from 1 for another, decided per table --; and the 2 + k words of the shared cells,
 *   packed: shared[q * n_shared + i] = acc[q * n_cells + shared_idx[i]].
 * Errors as the weighted calls'; k outside 1..8 or null weights: GCN10_E_INVAL; no weights: GCN10_E_STATE.  On a context
 * with more than one table gcn10_gpu_grid_sums_weighted / _finish_weighted answer GCN10_E_STATE and name these calls. */
#define GCN10_GPU_MAX_WEIGHT_TABLES 8
int gcn10_gpu_set_weight_tables(gcn10_gpu_ctx *ctx, const uint16_t *w /* [k][256] */, int k);
int gcn10_gpu_grid_sums_storms(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                               const int32_t *cellx_dev, const int32_t *celly_dev, int ncx, int ncy,
                               unsigned cond_mask, unsigned table_mask,
                               unsigned long long *acc /* [n_sel][ncy][ncx][2 + k] */, gcn10_stream_t stream);
int gcn10_gpu_grid_finish_storms(gcn10_gpu_ctx *ctx, const unsigned long long *acc, int n_sel, size_t n_cells,
                                 uint8_t *means, uint8_t *cnq /* [k][n_sel][n_cells] */,
                                 const uint32_t *shared_idx_dev, uint32_t n_shared,
                                 unsigned long long *shared /* [n_sel][n_shared][2 + k] */, gcn10_stream_t stream);

/* A weight table per cell (config key rain=...: a rainfall raster on the model grid).  Added in ABI 3 without a version
 * change, as the storms calls were; the host looks them up for rain runs only.
 *
 * gcn10_gpu_set_rain_tables: w[k][256], 1 <= k <= GCN10_GPU_MAX_RAIN_TABLES tables of 16-bit weights per raster value
 *   (host memory; w[t][255] is never read), kept on the device with a "never decreases over 1..100" flag per table.
 *   Synchronous.  Independent of gcn10_gpu_set_weights / gcn10_gpu_set_weight_tables: neither invalidates the other,
 *   and a later gcn10_gpu_set_tables does not invalidate the rain tables either -- they are functions of the value,
 *   not of the lookups, and nothing is folded.
 * gcn10_gpu_grid_sums_rain: every word of gcn10_gpu_grid_sums_weighted -- the maps, the -1 rule, ADD semantics, nothing
 *   read at or beyond W, nothing written outside acc whatever the maps hold, cells of 8 pixels or more --: words 0 and
 *   1 are exactly what gcn10_gpu_grid_sums adds, word 2 gets the sum of w[cell_table[cy * ncx + cx]][v] over the same
 *   pixels of cell (cx, cy).  cell_table_dev[ncy][ncx] names the table of every cell; an entry >= k is an error of the
 *   caller and counts as table 0.  There is no limit on the cell columns a workgroup meets, and pixels of a map whose
 *   entries do decrease are summed all the same.  The kernel works in items of GCN10_GPU_RAIN_ITEM_COLS columns x at
 *   most GCN10_GPU_RAIN_ITEM_ROWS rows, one wave each; a cell larger than an item gets its words from several.
 * gcn10_gpu_grid_finish_rain: means[] as gcn10_gpu_grid_finish writes it; cnq[q * n_cells + c] = the value of the
 *   triple by the rule of gcn10_runoff_cn with table cell_table[c] (c = cy * ncx + cx; an entry >= k counts as 0) --
 *   bisection for a table that never decreases, a scan from 1 for one that does, the table read from device memory --;
 *   and the triples of the shared cells, packed as gcn10_gpu_grid_finish_weighted packs them.
 * gcn10_gpu_grid_rain_item: the columns and rows of an item (either pointer may be NULL); returns their product, the
 *   most pixels a wave counts in 16 bits.  No device needed.
 * Errors as the weighted calls', cell_table among the pointers; k outside 1..256 or null weights: GCN10_E_INVAL; no rain
 * tables: GCN10_E_STATE ("call gcn10_gpu_set_rain_tables first"). */
#define GCN10_GPU_MAX_RAIN_TABLES 256
#define GCN10_GPU_RAIN_ITEM_COLS 512
#define GCN10_GPU_RAIN_ITEM_ROWS 127
int gcn10_gpu_grid_rain_item(int *cols, int *rows);
int gcn10_gpu_set_rain_tables(gcn10_gpu_ctx *ctx, const uint16_t *w /* [k][256] */, int k);
int gcn10_gpu_grid_sums_rain(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                             const int32_t *cellx_dev, const int32_t *celly_dev, int ncx, int ncy,
                             unsigned cond_mask, unsigned table_mask, const uint8_t *cell_table_dev /* [ncy][ncx] */,
                             unsigned long long *acc /* [n_sel][ncy][ncx][3] = {s, n, sw} */, gcn10_stream_t stream);
int gcn10_gpu_grid_finish_rain(gcn10_gpu_ctx *ctx, const unsigned long long *acc, int n_sel, size_t n_cells,
                               const uint8_t *cell_table_dev, uint8_t *means, uint8_t *cnq,
                               const uint32_t *shared_idx_dev, uint32_t n_shared, unsigned long long *shared,
                               gcn10_stream_t stream);

/* Several weight tables per cell (config key rains=...: 1 to GCN10_GPU_MAX_RAIN_LAYERS rainfall rasters on the model
 * grid, counted once).  Added in ABI 3 without a version change; the host looks them up for rains runs only.  The tables
 * are those of gcn10_gpu_set_rain_tables, which serves both pairs of calls; only the byte of a cell differs from layer to
 * layer.
 *
 * gcn10_gpu_grid_sums_rains: every word of gcn10_gpu_grid_sums_rain's contract -- the maps and the -1 rule, ADD
 *   semantics, any maps are summed (those whose entries decrease too), nothing at or beyond W is read, nothing outside
 *   acc is written, an entry >= the number of rain tables counts as table 0 --, for 2 + k words per (raster, cell): words
 *   0 and 1 are exactly what gcn10_gpu_grid_sums adds, word 2 + j gets the sum of w[cell_tables[j][cy * ncx + cx]][v]
 *   over the same pixels of cell (cx, cy).  cell_tables_dev holds k x ncy x ncx bytes and not one more is read.  The
 *   pixels are counted once whatever k is; the items and the launch are those of gcn10_gpu_grid_sums_rain.  With k = 1
 *   the call adds the words gcn10_gpu_grid_sums_rain adds.
 * gcn10_gpu_grid_finish_rains: means[] as gcn10_gpu_grid_finish writes it; cnq[(j * n_sel + q) * n_cells + c] = the value
 *   of {word 0, word 1, word 2 + j} by the rule of gcn10_runoff_cn with table cell_tables[j][c] (an entry >= the number
 *   of tables counts as 0), bisection or the scan by the table's flag as gcn10_gpu_grid_finish_rain; and the 2 + k words
 *   of the shared cells, packed as gcn10_gpu_grid_finish_storms packs them.  With k = 1 it writes the bytes and words of
 *   gcn10_gpu_grid_finish_rain.
 * Errors as the _rain calls'; k outside 1..GCN10_GPU_MAX_RAIN_LAYERS or null cell_tables: GCN10_E_INVAL naming the call;
 * no rain tables: GCN10_E_STATE ("call gcn10_gpu_set_rain_tables first").  A refused call writes nothing. */
#define GCN10_GPU_MAX_RAIN_LAYERS 8
int gcn10_gpu_grid_sums_rains(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                              const int32_t *cellx_dev, const int32_t *celly_dev, int ncx, int ncy,
                              unsigned cond_mask, unsigned table_mask,
                              const uint8_t *cell_tables_dev /* [k][ncy][ncx] */, int k,
                              unsigned long long *acc /* [n_sel][ncy][ncx][2 + k] */, gcn10_stream_t stream);
int gcn10_gpu_grid_finish_rains(gcn10_gpu_ctx *ctx, const unsigned long long *acc, int n_sel, size_t n_cells,
                                const uint8_t *cell_tables_dev /* [k][n_cells] */, int k, uint8_t *means,
                                uint8_t *cnq /* [k][n_sel][n_cells] */, const uint32_t *shared_idx_dev,
                                uint32_t n_shared, unsigned long long *shared /* [n_sel][n_shared][2 + k] */,
                                gcn10_stream_t stream);

/* A weight table per piece of a zone (config key zone_rain=...: a rainfall raster under the zones).  Added in ABI 3
 * without a version change; the host looks it up for zone_rain runs only.
 *
 * gcn10_gpu_zonal_sums_rain: esa, W, rows, cj, the prepared soil, the spans and what the caller guarantees of them are
 *   those of gcn10_gpu_zonal_pair_histogram; the tables are those of gcn10_gpu_set_rain_tables.  items_dev[i] names
 *   n_spans consecutive spans of ONE zone from first_span on, all under table `table` (gcn10_zone_rain_cut of
 *   gcn10_host.h makes spans and items, sorted by (zone, table)); `reserved` is not read; a table >= k is an error of
 *   the caller and counts as table 0.  ADDS, for every selected raster q (ascending raster order), every item and every
 *   pixel of its spans with value v != 255 -- v what gcn10_gpu_cn_strip writes for that raster at that pixel --, v to
 *   acc[zone][q][0], 1 to ...[1] and w[table][v] to ...[2].  Integers in 64 bits throughout the reduction: the triples
 *   do not depend on the launch shape, on how the spans are cut into items, or on order; the pixels of one (zone,
 *   table) run of a workgroup are counted in 32-bit words, so such a run names fewer than 2^32 pixels.  Pixels named by
 *   two spans count twice.  Any W, any alignment of esa; nothing at or beyond esa + W * rows is read; nothing outside
 *   acc's n_zones * n_sel * 3 words is written.  n_items == 0 is a successful no-op.  A workgroup takes a contiguous
 *   run of items; the grid is capped as gcn10_gpu_zonal_pair_histogram's.
 * GCN10_E_INVAL: the masks, W, rows or n_zones <= 0, a null pointer, n_items >= 2^32.  GCN10_E_STATE: no tables, no tile
 *   prepared for width W, or no rain tables ("call gcn10_gpu_set_rain_tables first").  Asynchronous on `stream`. */
#ifndef GCN10_ZONE_RAIN_ITEM_DEFINED
#define GCN10_ZONE_RAIN_ITEM_DEFINED
typedef struct gcn10_zone_rain_item { uint32_t first_span, n_spans, table, reserved; } gcn10_zone_rain_item;
#endif
int gcn10_gpu_zonal_sums_rain(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                              const gcn10_zone_span *spans_dev, const gcn10_zone_rain_item *items_dev, size_t n_items,
                              int n_zones, unsigned cond_mask, unsigned table_mask,
                              unsigned long long *acc /* [n_zones][n_sel][3] = {s, n, sw} */, gcn10_stream_t stream);

/* A tuple of weight tables per piece of a zone (config key zone_rains=...: 1 to GCN10_GPU_MAX_RAIN_LAYERS rainfall rasters
 * under the zones, counted once).  Added in ABI 3 without a version change; the host looks it up for zone_rains runs only.
 *
 * gcn10_gpu_zonal_sums_rains: every word of gcn10_gpu_zonal_sums_rain's contract -- esa, W, rows, cj, the prepared soil,
 *   the spans, ADD semantics, any W and any alignment of esa, nothing at or beyond esa + W * rows is read, pixels named
 *   twice count twice, the words do not depend on the launch shape, on how the spans are cut into items, or on order, a
 *   (zone, tuple) run of a workgroup names fewer than 2^32 pixels, n_items == 0 is a successful no-op that reads no
 *   pointer --, for 2 + k words per (zone, raster): words 0 and 1 are s and n, word 2 + j gets the sum of
 *   w[items_dev[i].table[j]][v] over the item's pixels with v != 255.  items_dev[i] names n_spans consecutive spans of ONE
 *   zone from first_span on, all under ONE tuple (gcn10_zone_rains_cut of gcn10_host.h makes spans and items, sorted by
 *   (zone, tuple)).  A byte that is at least the number of rain tables counts as table 0.  Bytes k..7 of an item pick no
 *   table, and the words never depend on them.  Nothing outside acc's n_zones * n_sel * (2 + k) words is written.  The
 *   pixels are counted once whatever k is.  With k = 1 the call adds exactly the words gcn10_gpu_zonal_sums_rain adds for
 *   table = table[0].  The grid is capped as that call's.
 * GCN10_E_INVAL naming the call: k outside 1..GCN10_GPU_MAX_RAIN_LAYERS, or any argument the one-raster call refuses.
 *   GCN10_E_STATE: no tables, no tile prepared for width W, or no rain tables.  A refused call writes nothing.
 *   Asynchronous on `stream`. */
#ifndef GCN10_ZONE_RAINS_ITEM_DEFINED
#define GCN10_ZONE_RAINS_ITEM_DEFINED
typedef struct gcn10_zone_rains_item { uint32_t first_span, n_spans; uint8_t table[8]; } gcn10_zone_rains_item;
#endif
int gcn10_gpu_zonal_sums_rains(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                               const gcn10_zone_span *spans_dev, const gcn10_zone_rains_item *items_dev, size_t n_items,
                               int n_zones, unsigned cond_mask, unsigned table_mask, int k,
                               unsigned long long *acc /* [n_zones][n_sel][2 + k] = {s, n, sw_1 .. sw_k} */,
                               gcn10_stream_t stream);

/* Verification of written rasters (config key verify=1): decoded file rasters compared on the GPU with the values
 * computed now.  Added in ABI 3 without a version change; the host looks them up for verify runs only.
 *
 * gcn10_gpu_verify_strip: same contract for `esa`, `cj`, the masks and the soil prepared by gcn10_gpu_prepare_tile
 *   as gcn10_gpu_cn_strip, for rows [y0, y0 + rows) of the block.  got[r] (host array of device pointers; entries of
 *   unselected rasters are ignored) is the decoded strip of raster r, rows got_stride >= W bytes apart; bytes
 *   beyond column W are never read and nothing is written to got.  The call ADDS to counts_dev[GCN10_N_RASTERS]:
 *   clear it once per block -- mismatches = 0, first = UINT64_MAX (gcn10_gpu_memset with 0xff, then the counters
 *   with 0, or a copy of such an array).  Entries of unselected rasters are left alone.  `first` is the minimum over
 *   everything added so far in row-major order, so it does not depend on strip size or launch shape; want / got
 *   are those of the pixel `first` names, written by a second small launch when that pixel lies in this call's
 *   rows.  The calls that add to one counts_dev must therefore be ordered (one stream, or events).
 * gcn10_gpu_verify_buffers: the same counting for rasters whose expected pixels exist in device memory (the
 *   average overviews): want[r] against got[r], W x rows pixels each with their own row strides, for the rasters
 *   of raster_mask (bit r). */
typedef struct gcn10_verify_count {
    uint64_t mismatches;        /* pixels of this raster whose file value differs from the computed one */
    uint64_t first;             /* smallest (y << 32 | x) among them, block coordinates; UINT64_MAX if none */
    uint32_t want, got;         /* computed value and file value at `first` */
} gcn10_verify_count;
int gcn10_gpu_verify_strip(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                           unsigned cond_mask, unsigned table_mask,
                           const uint8_t *const got[GCN10_N_RASTERS], size_t got_stride, int y0,
                           gcn10_verify_count *counts_dev, gcn10_stream_t stream);
int gcn10_gpu_verify_buffers(gcn10_gpu_ctx *ctx, const uint8_t *const want[GCN10_N_RASTERS], size_t want_stride,
                             const uint8_t *const got[GCN10_N_RASTERS], size_t got_stride, int W, int rows, int y0,
                             unsigned raster_mask, gcn10_verify_count *counts_dev, gcn10_stream_t stream);

/* Launch-shape knobs of the strip kernels, for tuning runs; results never
 * depend on them.  Names: "grid_blocks_per_cu" (1..64), "ilp16" (0 = by raster count | 1 | 2),
 * "ilp1" (1|2|4), "nontemporal" (0|1), "xcd_slabs" (0|1), "prefetch" (software pipeline of the strip kernels: -1 = default = on | 0 | 1), "compact_soil" (0|1: strips of
 * 16-byte aligned rows read the cell codes and the column map of the prepared tile, not its code bytes; takes effect with the next
 * strip, no new gcn10_gpu_prepare_tile needed; default 1), "deflate_wave_codes" (0|1: code
 * construction of the tile encoder by one thread or one wave per tile), "defaults" (value
 * ignored: every knob back to its built-in default).
 * Round 3: "arena_segment_align" (16..4096, a power of two; default 4096: every raster's extent of a strip starts at a
 * multiple of it in the arena), "fused_parse" / "fused_emit" (0 = the round-2 forms of the fused encoder's first and
 * last pass, kept as cross-checks; 1 = default; the streams are the same bytes), "event_sync_sleep_us" (0 = default: gcn10_gpu_event_sync
 * is hipEventSynchronize, which spins; n > 0: it queries the event and sleeps n microseconds in between -- what a
 * host pipeline's waiting threads want). */
int gcn10_gpu_set_option(gcn10_gpu_ctx *ctx, const char *name, int value);

/* The rasters of a strip through a byte table per cell of a coarse grid (config key runoff_rain=...: the per-pixel runoff
 * depth under a rainfall raster).  Added in ABI 3 without a version change, as the rain calls were; the host looks them
 * up for runoff_rain runs only.
 *
 * gcn10_gpu_set_cell_byte_tables: t[k][256], 1 <= k <= GCN10_GPU_MAX_CELL_BYTE_TABLES tables of bytes per raster value
 *   (copied).  Synchronous.  Independent of the weight and the rain tables, and a later gcn10_gpu_set_tables does not
 *   invalidate them -- they are functions of the value, not of the lookup tables.  A second call replaces the first.
 * gcn10_gpu_runoff_strip: esa, W, rows, cj, the masks, out[] and the prepared tile are those of gcn10_gpu_cn_strip
 *   (unselected entries of out[] are ignored; out[] must be ordinary device allocations).  cellx_dev[W] and
 *   celly_dev[rows] are the maps of gcn10_gpu_grid_sums_rain, celly pointing at the strip's first row: an entry outside
 *   0..ncx-1 or 0..ncy-1 means "in no cell"; no minimum cell size and no order are assumed -- entries may decrease or
 *   repeat, and a cell may be one pixel wide.  For every selected raster r and pixel (x, y), with v what
 *   gcn10_gpu_cn_strip writes there:
 *       out[r][y * W + x] = T[cell_table[celly[y] * ncx + cellx[x]]][v]    if both maps name a cell,
 *                           255                                            otherwise;
 *   a cell_table entry >= k counts as table 0, the rule of the rain sums.  The library applies T as given, T[t][255]
 *   included: it knows nothing about runoff.  Any W >= 1, any alignment of esa and out[]; nothing at or beyond W * rows
 *   is read or written in any raster; cutting the rows into several calls gives the same bytes.  Asynchronous on
 *   `stream`; the call expands cell_table through cellx into a workspace of the context first (2 bytes per column and
 *   cell row, on `stream`), so the calls of one context are made on one stream or ordered by the caller.  Honours
 *   gcn10_gpu_time_next_strip (the strip kernel, not the expansion).
 *   Kernel names in profiles: runoff_strip_kernel<256> (k <= 32), runoff_strip_kernel<1024>, expand_cell_tables_kernel.
 * Errors: GCN10_E_INVAL: bad masks, W, rows, ncx or ncy <= 0, more than 2^31-1 pixels, null pointers (a selected out[r]
 *   among them), k outside 1..256 or null tables; GCN10_E_STATE: no lookup tables, no tile prepared for W, no byte tables
 *   ("call gcn10_gpu_set_cell_byte_tables first"), or a device whose workgroups cannot hold the tables in LDS.  A
 *   refused call writes nothing. */
#define GCN10_GPU_MAX_CELL_BYTE_TABLES 256
int gcn10_gpu_set_cell_byte_tables(gcn10_gpu_ctx *ctx, const uint8_t *t /* [k][256] */, int k);
int gcn10_gpu_runoff_strip(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                           const int32_t *cellx_dev, const int32_t *celly_dev, int ncx, int ncy,
                           const uint8_t *cell_table_dev /* [ncy][ncx] */,
                           unsigned cond_mask, unsigned table_mask,
                           uint8_t *const out[GCN10_N_RASTERS], gcn10_stream_t stream);

/* Measurement: the next gcn10_gpu_cn_strip launch records `start` / `stop` as part of
 * the kernel dispatch itself (hipExtLaunchKernel), so gcn10_gpu_event_elapsed_ms gives
 * the kernel's own duration -- the figure rocprofv3 --kernel-trace reports. One shot. */
int gcn10_gpu_time_next_strip(gcn10_gpu_ctx *ctx, gcn10_event_t start, gcn10_event_t stop);

/* Measurement: a plain copy of `bytes` (a multiple of 16, both pointers 16-byte aligned)
 * from `src` to `dst`, with the strip kernel's launch shape and nothing but the two
 * streams: what this device sustains for 1 byte read : 1 byte written.  bench.py times
 * it next to the strip kernel, in the same run.  Honours gcn10_gpu_time_next_strip.
 * Kernel name in profiles: stream_copy_kernel.  No counterpart in the reference. */
int gcn10_gpu_stream_copy(gcn10_gpu_ctx *ctx, const void *src, void *dst, size_t bytes,
                          gcn10_stream_t stream);

/* Placement and launch-shape calibration for one-raster strips (BASELINE config 2 / config 3).
 * A strip with one raster is a 1 byte read : 1 byte written stream, and on MI355X the rate of such a
 * stream depends on where the written buffer lies relative to the read one -- periodically in the
 * distance, with a 128 MiB period for a grid-stride sweep, by up to 20 % (DESIGN.md section 5,
 * profiles/r02/offset_lab_*.jsonl) -- and the best workgroup -> address mapping depends on it too.
 * The call times the single-raster kernel of (cond_mask, table_mask: one bit each) on this very
 * landcover strip for every position arena + i * step (step a multiple of 256; while a raster of
 * W * rows bytes still fits in arena_bytes) and a fixed set of launch shapes, keeps the fastest
 * shape for later single-raster launches of this context (the all-tables kernel is not affected;
 * gcn10_gpu_set_option "ilp1" or "defaults" drops it) and returns the fastest position.
 * The arena is caller-owned device memory; its contents are overwritten.  `report` (optional)
 * receives a one-line JSON summary.  Results of later launches do not depend on any of this.
 * Synchronises `stream`.  No counterpart in the reference (its buffers are malloc'ed per raster,
 * src/cn.c:264,278). */
int gcn10_gpu_tune_single_raster(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows,
                                 const int32_t *cj, unsigned cond_mask, unsigned table_mask,
                                 uint8_t *arena, size_t arena_bytes, size_t step,
                                 uint8_t **best_out, float *best_ms, char *report, size_t report_cap,
                                 gcn10_stream_t stream);

/* What the strips of the tile last prepared on this context read their soil codes from (synchronises
 * `stream`, on which gcn10_gpu_prepare_tile ran): 0 = code bytes (tables switched off with
 * gcn10_gpu_set_option("compact_soil", 0)), 1 = one column entry per lane -- every 16-pixel column group of the tile
 * is a run of one soil column followed by a run of another, and a lane of a strip whose width is a multiple of 16
 * keeps its group's entry for the whole launch and loads two cell codes per 16 pixels --, 2 = the cell codes through
 * the column map, pixel by pixel, because some column group of this tile has no such form (more than two soil cells,
 * a map that is not monotone).  The answer describes the tile, as before: a strip of another width, or one with
 * more column groups in a row than its launch has threads, reads the code bytes whatever it says.  <0 on error.  A
 * diagnostic: nothing needs to call it. */
int gcn10_gpu_soil_words_state(gcn10_gpu_ctx *ctx, gcn10_stream_t stream);

/* Name of the variant of the strip kernel the last cn_strip call launched
 * (for profiles and bench records). */
const char *gcn10_gpu_last_kernel_name(gcn10_gpu_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* GCN10_GPU_H */
