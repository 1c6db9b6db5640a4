// gcn10_gpu_internal.hpp -- shared by the translation units of libgcn10_gpu.so.
#ifndef GCN10_GPU_INTERNAL_HPP
#define GCN10_GPU_INTERNAL_HPP

#include <hip/hip_runtime.h>

#include <cstdint>

#include "gcn10_gpu.h"
#include "gcn10_strip_lanes.hpp"

namespace gcn10 {

// error plumbing: message of the calling thread (gcn10_gpu_last_error)
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return gcn10::fail(e_ == hipErrorOutOfMemory ? GCN10_E_NOMEM : GCN10_E_HIP, \
                               "%s: %s", #expr, hipGetErrorString(e_));                 \
    } while (0)

// ---- gcn10_context.hip ----
int use_device(gcn10_gpu_ctx *ctx);
hipStream_t as_stream(gcn10_gpu_ctx *ctx, gcn10_stream_t s);
// Grows one of the context's device workspaces (*ws of *cap bytes) to at least `need` bytes; the old
// contents are not kept.
int grow_workspace(void **ws, size_t *cap, size_t need);
// the most workgroups a reader that loops over its work launches: per_cu on every compute unit
uint32_t grid_cap(const gcn10_gpu_ctx *ctx, int per_cu);
// Memory-bound streaming grid: a few workgroups per CU, each looping over
// chunks; a multiple of 8 so every XCD gets the same number.
uint32_t stream_grid(const gcn10_gpu_ctx *ctx, uint64_t nchunks, int blocks_per_cu = 0);
// Launches a kernel of kThreads threads.  A pair of events left by gcn10_gpu_time_next_strip is attached to the
// dispatch itself (they bracket the kernel, not the command-processor gaps around separately recorded events) and
// used up.
hipError_t launch_timed(gcn10_gpu_ctx *ctx, const void *fn, uint32_t grid, void **args, hipStream_t s);

// ---- the host preamble of the soil readers (gcn10_soil_readers.hpp has their device side) ----
struct SoilView;
// gcn10_tables.hip: GCN10_E_STATE unless gcn10_gpu_set_tables has run
int check_tables(gcn10_gpu_ctx *ctx, const char *who);
// GCN10_E_INVAL unless the masks name at least one condition and one loaded table, and nothing else
int check_masks(gcn10_gpu_ctx *ctx, const char *who, unsigned cond_mask, unsigned table_mask);
// gcn10_soil_tile.hip: GCN10_E_STATE unless a tile is prepared
int check_tile(gcn10_gpu_ctx *ctx, const char *who);
// The soil code bytes of the prepared tile (gcn10_gpu_ctx::Tile::d_hx), valid for work that `stream` runs after this
// call: the first caller after a gcn10_gpu_prepare_tile expands them from the tile's tables on its own stream, every
// later caller's stream is made to wait for that expansion (no cost on the stream that ran it).  prepare_tile and
// bind_soil call it, with a tile prepared; every kernel that reads the bytes gets them through bind_soil.
int soil_bytes(gcn10_gpu_ctx *ctx, hipStream_t stream, const uint8_t **hx);
// GCN10_E_STATE unless a tile is prepared, and for width W; then the view of its code bytes (soil_bytes on `stream`)
// for a strip whose rows cj maps
int bind_soil(gcn10_gpu_ctx *ctx, const char *who, int W, hipStream_t stream, const int32_t *cj, SoilView *view);

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// soil code byte of the hx workspace: drained plane | undrained plane << 4, planes 0..5;
// compact index = drained * 6 + undrained
constexpr int kClassCodes = 36;

}  // namespace gcn10

struct gcn10_gpu_ctx {
    int device = -1;
    int n_cus = 0;
    hipStream_t main_stream = nullptr;

    // ---- the tables (gcn10_tables.hip) ----
    uint8_t *d_lut16 = nullptr;     // kLut16Bytes: the all-tables image (gcn10_soil_readers.hpp)
    uint8_t *d_lut1 = nullptr;      // 9 * kLut1Bytes
    int n_tables = 0;
    uint8_t *d_class_of = nullptr;  // [36][256] pixel class of (soil code, landcover), then [18][256] values
    int n_classes = 0;              // 0: not available (set_tables not called, or > 256 classes)

    // ---- the weights of the weighted grid sums (gcn10_grid.hip: gcn10_gpu_set_weights) ----
    uint8_t *d_wlut = nullptr;      // per table two images of the all-tables layout, the low and the high bytes of
                                    // w[cn] (0 where d_lut16 holds 255), then the n_weights tables w[256] themselves
    bool weights_set = false;       // ... are those of the loaded tables (gcn10_gpu_set_tables clears it)
    int n_weights = 0;              // tables of weights: 1 (gcn10_gpu_set_weights) to GCN10_GPU_MAX_WEIGHT_TABLES
    uint32_t weights_rising = 0;    // bit j: w_j[1..100] never decrease

    // ---- the tables of the rain sums (gcn10_grid_rain.hip: gcn10_gpu_set_rain_tables) ----
    uint16_t *d_rain_tables = nullptr;  // n_rain_tables tables w[256], then a byte per table: w[1..100] never decrease
    int n_rain_tables = 0;              // 0: not set

    // ---- the byte tables of the per-cell strips (gcn10_runoff_strip.hip: gcn10_gpu_set_cell_byte_tables) ----
    uint8_t *d_cell_byte_tables = nullptr;  // n_cell_byte_tables tables of 256 bytes, then 256 bytes 255 ("in no cell")
    int n_cell_byte_tables = 0;             // 0: not set

    // ---- the prepared tile (gcn10_soil_tile.hip) ----
    struct Tile {
        // Soil workspace of the prepared tile (one allocation, grown by gcn10_gpu_prepare_tile):
        //   d_hx      [hx_rows][hx_stride]      soil code bytes, one per fine column.  Allocated with the tile, FILLED ON
        //                                        DEMAND: every reader gets them as a gcn10::SoilView from bind_soil()
        //   d_cx      [hx_stride]               clamped coarse column of every fine column; hsx = padding
        //   d_codes   [hx_rows][codes_stride]   soil code of every coarse cell; columns >= hsx hold the padding code
        // d_cx and d_codes are a snapshot of the caller's `coarse` and `ci`: nothing reads those after prepare_tile.  The
        // strips of 16-byte aligned rows read them directly (one column group per lane), the other readers the bytes.
        uint8_t *d_hx = nullptr;        // row 0 of the soil-code bytes (= d_hx_alloc + 16)
        void *d_hx_alloc = nullptr;
        size_t hx_capacity = 0;         // of d_hx_alloc, the 16 bytes in front of row 0 included
        uint32_t hx_stride = 0;
        uint32_t hx_W = 0;
        uint32_t hx_rows = 0;
        uint32_t *d_cx = nullptr;
        uint8_t *d_codes = nullptr;
        uint32_t codes_stride = 0;
        uint32_t *d_soil_complex = nullptr;  // device word: == soil_gen when some group of the prepared tile has no compact form
        uint32_t soil_gen = 0;               // generation number of the prepared tile (never 0 once a tile is prepared)
        bool hx_made = false;               // the bytes of the prepared tile have been launched ...
        hipEvent_t hx_made_ev = nullptr;    // ... and this event follows them
    } tile;

    // launch shape of the single-table strip kernel as gcn10_gpu_tune_single_raster left it (the knobs
    // of Options keep steering the all-tables kernel)
    struct SingleShape {
        bool set = false;
        int xcd_slabs = 1, grid_blocks_per_cu = 8, ilp = 2, prefetch = 1;
    };

    // ---- everything gcn10_gpu_set_option writes; "defaults" assigns a fresh one (gcn10_context.hip) ----
    struct Options {
        // strip tuning knobs; defaults = the round-1 measured best
        int grid_blocks_per_cu = 16;
        int ilp16 = 0;          // sub-chunks per loop trip, all-tables kernel (1, 2; 0 = by stream count)
        int ilp1 = 2;           // same, single-table kernel (1, 2, 4)
        int nontemporal = 1;
        int xcd_slabs = 1;
        int prefetch = 1;       // software pipeline: loads of the next trip issued before the current one is
                                // consumed (two register sets; -1 = default = on)
        int compact_soil = 1;               // aligned strips read the tables, not the bytes
        SingleShape single;
        int arena_segment_align = 4096; // tile encoder: a raster's streams of a strip start at a multiple of this (16 .. 4096)
        int deflate_wave_codes = 1;     // pass B of the tile encoder: 1 = one wave per tile, 0 = one thread
        int fused_parse = 1;            // pass F-A of the fused encoder: 1 = one lane per 64-pixel segment (round 3), 0 = one lane per row
        int fused_emit = 1;             // pass F-C of the fused encoder: 1 = every wave packs its own quarter of the tokens (round 3), 0 = lock step
        int event_sync_sleep_us = 0;    // gcn10_gpu_event_sync: 0 = hipEventSynchronize (spins); n > 0 = query, sleep n us, query ...
    } opt;

    const char *last_kernel = "";   // of the last strip (a string of the strip-kernel table)
    hipEvent_t time_start = nullptr, time_stop = nullptr;  // one-shot: bracket the next strip kernel
    // dynamic-LDS attributes set on this device (gcn10::allow_dynamic_lds), each by the file that owns the kernels
    bool deflate_ready = false;         // passes A and C (gcn10_deflate.hip)
    bool codes_ready = false;           // the per-thread form of pass B (gcn10_deflate_codes.hip)
    bool fused_stats_ready = false;     // pass F-A (gcn10_deflate_fused_stats.hpp)
    bool fused_emit_ready = false;      // pass F-C (gcn10_deflate_fused_emit.hpp)
    bool runoff_strip_ready = false;    // gcn10_runoff_strip.hip

    // ---- device workspaces of the codecs, grown by gcn10::grow_workspace ----
    struct Workspaces {
        void *deflate = nullptr;    // per-tile statistics + code books of the tile encoder
        size_t deflate_cap = 0;
        void *inflate = nullptr;    // linear slots of the tiles being decoded (gcn10_inflate.hip)
        size_t inflate_cap = 0;
        void *lzw = nullptr;        // segment bit strings + their lengths of the LZW tile encoder (gcn10_lzw.hip)
        size_t lzw_cap = 0;
        void *cell_tables = nullptr;    // the table of every (cell row, fine column) of a per-cell strip (gcn10_runoff_strip.hip)
        size_t cell_tables_cap = 0;
    } ws;
};

#endif
