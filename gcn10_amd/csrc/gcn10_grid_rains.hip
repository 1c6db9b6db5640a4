// gcn10_grid_rains.hip -- the words {s, n, sw_1 .. sw_k} of every selected raster over the cells of a model grid, with k
// weight tables chosen PER CELL, one per layer of rainfall (config key rains=..., DESIGN.md "Several rainfall rasters").
//
// The pixels are counted as gcn10_grid_rain.hip counts them and by the same code (gcn10_grid_rain_piece.hpp): a wave
// owns an item of kItemCols x at most kItemRows pixels, walks the pieces of cells in it, counts a piece into the pair
// histogram in LDS and packs the non-zero bins to its front.  Only what follows depends on the tables, and it is done
// once per WORD rather than once per piece, so that k layers cost one count and 2 + k short reductions:
//
//   - a lane keeps its first packed bin -- the count and the two 16-byte rows of the all-tables image that give the
//     value of every raster for the bin's pair -- in registers across the words.  A piece packs a few dozen bins, so
//     that is usually all a lane has; the bins beyond the 64th of a piece stay packed in LDS and are met again there,
//     with their image rows, for every word (kWave, 2 kWave, ... behind the lane);
//   - for one word at a time a lane adds up 18 partial sums, (condition, table), and the wave adds each over its 64
//     lanes with DPP adds (wave_total): no LDS is written, so the packed bins outlive every word whatever their
//     number, and there is nothing to transpose or to clear between the layers.  The DPP adds leave a total in
//     the last 16 lanes: lane 48 + t takes that of table t and issues ONE 64-bit atomic add per non-zero (raster,
//     word) of the piece;
//   - the k bytes of the cell are read once per piece, the byte of the next layer while this one is reduced.
//
// The packed bins are cleared when the piece ends.  Registers: 18 sums, the bin and its rows -- the 2 x 9 x (2 + k) sums
// of a piece never exist at once.  Layers with equal bytes in a cell are reduced again, not recognised.
//
// The launch is that of gcn10_gpu_grid_sums_rain: one workgroup per item, bands of band_height(ctx, 16, chunks, rows,
// 16, 127) rows.  gcn10_gpu_grid_finish_rains is one thread per (raster, cell) with a loop over the layers.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gcn10_grid_internal.hpp"
#include "gcn10_grid_rain_piece.hpp"
#include "gcn10_wave.hpp"

using namespace gcn10;
using namespace gcn10::rain_piece;

namespace {

constexpr uint32_t kTotalLane = 48u;                        // wave_total_in_last_row: lanes 48..56 take the 9 tables' sums
constexpr int kFinishThreads = 256;

struct RainsParams {
    const uint8_t *esa;             // strip, W x rows, row major
    SoilView soil;                  // soil code bytes, soil row of every strip row
    const uint8_t *lut;             // the all-tables image, in global memory
    const int32_t *cellx, *celly;
    const uint8_t *cell_tables;     // [k][ncy][ncx]: the table of every cell in every layer
    const uint16_t *tables;         // [n_tables][256]
    uint32_t n_tables, k;
    uint32_t W, rows, ncx, ncy;
    uint32_t chunks, band_rows;
    uint32_t sel;                   // bit r: raster r is selected
    uint32_t n_conds, conds[2];     // the selected conditions
    unsigned long long *acc;        // [n_sel][ncy][ncx][2 + k]
};

// a packed bin: its count, and per selected condition the image row of its pair (byte t: the value of table t)
struct Bin {
    uint32_t c;
    u32x4 row[2];
};

__device__ __forceinline__ void load_bin(const RainsParams &p, uint32_t ent, Bin &b)
{
    const uint32_t lc = (ent >> 16) & 255u, code = bin_code(ent >> 24);
    b.c = ent & 0xffffu;
#pragma unroll
    for (uint32_t ci = 0; ci < 2; ci++)
        if (ci < p.n_conds)
            b.row[ci] = *reinterpret_cast<const u32x4 *>(lut16_row(p.lut, (code >> (4u * p.conds[ci])) & 15u, lc));
}

enum : uint32_t { kWordS = 0u, kWordN = 1u, kWordSw = 2u };

// a bin's share of one word of every selected raster: c * v, c, or c * w[v]
template <uint32_t kind>
__device__ __forceinline__ void add_bin(const RainsParams &p, const Bin &b, const uint16_t *w,
                                        uint32_t (&sum)[2][9])
{
#pragma unroll
    for (uint32_t ci = 0; ci < 2; ci++) {
        if (ci >= p.n_conds)
            continue;
        const uint32_t sel9 = (p.sel >> (9u * p.conds[ci])) & 0x1ffu;
#pragma unroll
        for (uint32_t t = 0; t < 9; t++) {
            if (!((sel9 >> t) & 1u))            // wave uniform
                continue;
            // w has 256 entries: the weight is loaded for every lane, and counts for a valid value
            const uint32_t v = (b.row[ci][t >> 2] >> (8u * (t & 3u))) & 255u;
            const uint32_t x = kind == kWordS ? b.c * v : kind == kWordN ? b.c : b.c * w[v];
            sum[ci][t] += v != GCN10_NODATA ? x : 0u;
        }
    }
}

// One word of the piece's cell, for every selected raster: the lane's first bin from registers, its further bins (a
// piece of more than 64) from h[lane + 64 ..), the 18 sums added over the wave, one atomic per non-zero one.  Called by
// the whole wave; h is only read.
template <uint32_t kind>
__device__ __forceinline__ void add_word(const RainsParams &p, const uint32_t *h, uint32_t m, const Bin &first,
                                         const uint16_t *w, size_t cell, uint32_t word)
{
    const uint32_t lane = threadIdx.x;
    uint32_t sum[2][9];
#pragma unroll
    for (uint32_t ci = 0; ci < 2; ci++)
#pragma unroll
        for (uint32_t t = 0; t < 9; t++)
            sum[ci][t] = 0u;
    if (lane < m)
        add_bin<kind>(p, first, w, sum);
    for (uint32_t i = lane + kWave; i < m; i += kWave) {
        Bin b = {};
        load_bin(p, h[i], b);
        add_bin<kind>(p, b, w, sum);
    }
    // every lane is here again.  The sums of the whole piece fit 32 bits, as the item's do; lane kTotalLane + t takes
    // the wave's sum of table t, in one register per condition
    uint32_t total[2] = {0u, 0u};
#pragma unroll
    for (uint32_t ci = 0; ci < 2; ci++) {
        if (ci >= p.n_conds)                    // wave uniform, as the selection is
            continue;
        const uint32_t sel9 = (p.sel >> (9u * p.conds[ci])) & 0x1ffu;
#pragma unroll
        for (uint32_t t = 0; t < 9; t++) {
            if (!((sel9 >> t) & 1u))
                continue;
            const uint32_t all = wave_total_in_last_row(sum[ci][t]);
            if (lane == kTotalLane + t)
                total[ci] = all;
        }
    }
#pragma unroll
    for (uint32_t ci = 0; ci < 2; ci++)
        if (total[ci]) {                        // no lane of a condition or table that is not selected
            const uint32_t r = 9u * p.conds[ci] + (lane - kTotalLane);
            const uint32_t q = __popc(p.sel & ((1u << r) - 1u));
            atomicAdd(p.acc + ((size_t)q * p.ncy * p.ncx + cell) * (2u + p.k) + word, (unsigned long long)total[ci]);
        }
}

// Columns [xa, xb) x rows [ya, yb) of cell (cx, cy), all inside the wave's item: counted once, reduced for s, n and
// against the cell's table in every layer, and added to the cell's words.  h is all zero before and after.
__device__ __forceinline__ void sum_piece(const RainsParams &p, uint32_t *h, uint32_t xa, uint32_t xb, uint32_t ya,
                                          uint32_t yb, uint32_t cx, uint32_t cy)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t m = count_and_pack(p, h, xa, xb, ya, yb);
    if (m == 0u)
        return;                 // the same for the whole wave

    const size_t cell = (size_t)cy * p.ncx + cx, layer = (size_t)p.ncy * p.ncx;
    uint32_t tb = p.cell_tables[cell];          // layer 0's byte, under way while the bins are fetched
    Bin first = {};
    if (lane < m)
        load_bin(p, h[lane], first);
    add_word<kWordS>(p, h, m, first, nullptr, cell, 0u);
    add_word<kWordN>(p, h, m, first, nullptr, cell, 1u);
    for (uint32_t j = 0; j < p.k; j++) {
        const uint16_t *const w = p.tables + 256u * (tb < p.n_tables ? tb : 0u);
        if (j + 1u < p.k)
            tb = p.cell_tables[(j + 1u) * layer + cell];
        add_word<kWordSw>(p, h, m, first, w, cell, 2u + j);
    }
    for (uint32_t i = lane; i < m; i += kWave)  // the words this lane alone has read since the pack
        h[i] = 0u;
    __syncthreads();
}

__global__ __launch_bounds__(kWave) void grid_sums_rains_kernel(const RainsParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t h[kHistWords];
    walk_item(p, h, [&](uint32_t xa, uint32_t xb, uint32_t ya, uint32_t yb, uint32_t cx, uint32_t cy) {
        sum_piece(p, h, xa, xb, ya, yb, cx, cy);
    });
}

struct RainsFinishParams {
    const unsigned long long *acc;
    size_t n_cells;
    uint8_t *means, *cnq;
    const uint32_t *shared_idx;
    uint32_t n_shared;
    unsigned long long *shared;
    const uint8_t *cell_tables;     // [k][n_cells]
    const uint16_t *tables;         // [n_tables][256], then a byte per table: entries 1..100 never decrease
    uint32_t n_tables, k, n_sel;
};

// blockIdx.y: the raster; a thread: a cell, and a shared cell
__global__ __launch_bounds__(kFinishThreads) void grid_finish_rains_kernel(const RainsFinishParams p)
{
    const size_t q = blockIdx.y, i = (size_t)blockIdx.x * kFinishThreads + threadIdx.x;
    const uint32_t words = 2u + p.k;
    if (i < p.n_cells) {
        const unsigned long long *const a = p.acc + words * (q * p.n_cells + i);
        const unsigned long long s = a[0], n = a[1];
        const uint8_t *const rising = reinterpret_cast<const uint8_t *>(p.tables + 256u * p.n_tables);
        p.means[q * p.n_cells + i] = mean_byte(s, n);
        for (uint32_t j = 0; j < p.k; j++) {
            const uint32_t tb = p.cell_tables[j * p.n_cells + i], t = tb < p.n_tables ? tb : 0u;
            p.cnq[((size_t)j * p.n_sel + q) * p.n_cells + i] =
                runoff_cn(p.tables + 256u * t, rising[t] != 0, s, n, a[2u + j]);
        }
    }
    if (i < p.n_shared) {
        const unsigned long long *const a = p.acc + words * (q * p.n_cells + p.shared_idx[i]);
        unsigned long long *const to = p.shared + words * (q * p.n_shared + i);
        for (uint32_t j = 0; j < words; j++)
            to[j] = a[j];
    }
}

int check_layers(const char *who, const uint8_t *cell_tables, int k)
{
    if (!cell_tables || k < 1 || k > GCN10_GPU_MAX_RAIN_LAYERS)
        return fail(GCN10_E_INVAL, "%s: bad arguments k=%d (1..%d layers, no null cell_tables)", who, k,
                    GCN10_GPU_MAX_RAIN_LAYERS);
    return GCN10_OK;
}

}  // namespace

extern "C" {

int gcn10_gpu_grid_sums_rains(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                              const int32_t *cellx, const int32_t *celly, int ncx, int ncy, unsigned cond_mask,
                              unsigned table_mask, const uint8_t *cell_tables, int k, unsigned long long *acc,
                              gcn10_stream_t stream)
{
    const char *const who = "gcn10_gpu_grid_sums_rains";
    int rc = use_device(ctx);
    if (rc)
        return rc;
    hipStream_t s = as_stream(ctx, stream);
    RainsParams p = {};
    if ((rc = check_tables(ctx, who)) != GCN10_OK)
        return rc;
    if ((rc = check_rain_tables(ctx, who)) != GCN10_OK)
        return rc;
    if ((rc = bind_soil(ctx, who, W, s, cj, &p.soil)) != GCN10_OK)
        return rc;
    if ((rc = check_layers(who, cell_tables, k)) != GCN10_OK)
        return rc;
    if ((rc = check_sums_args(who, esa, W, rows, cj, cellx, celly, ncx, ncy, acc)) != GCN10_OK)
        return rc;
    if ((rc = check_masks(ctx, who, cond_mask, table_mask)) != GCN10_OK)
        return rc;
    // the LDS a workgroup may take, from the device
    int lds = 0;
    HIP_TRY(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
    if ((size_t)lds < kHistWords * sizeof(uint32_t))
        return fail(GCN10_E_STATE, "%s: the device gives a workgroup %d bytes of LDS, the histogram takes %zu", who, lds,
                    kHistWords * sizeof(uint32_t));
    p.esa = esa;
    p.lut = ctx->d_lut16;
    p.cellx = cellx;
    p.celly = celly;
    p.cell_tables = cell_tables;
    p.tables = ctx->d_rain_tables;
    p.n_tables = (uint32_t)ctx->n_rain_tables;
    p.k = (uint32_t)k;
    p.W = (uint32_t)W;
    p.rows = (uint32_t)rows;
    p.ncx = (uint32_t)ncx;
    p.ncy = (uint32_t)ncy;
    p.acc = acc;
    p.sel = select_rasters(cond_mask, table_mask, p.conds, p.n_conds);
    p.chunks = (p.W + kItemCols - 1u) / kItemCols;
    p.band_rows = band_height(ctx, 16, p.chunks, p.rows, kMinBandRows, kItemRows);
    const uint64_t grid = (uint64_t)((p.rows + p.band_rows - 1u) / p.band_rows) * p.chunks;
    if (grid > 0x7fffffffull)
        return fail(GCN10_E_INVAL, "%s: %llu workgroups; cut the strip into bands", who, (unsigned long long)grid);
    hipLaunchKernelGGL(grid_sums_rains_kernel, dim3((uint32_t)grid), dim3(kWave), 0, s, p);
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}

int gcn10_gpu_grid_finish_rains(gcn10_gpu_ctx *ctx, const unsigned long long *acc, int n_sel, size_t n_cells,
                                const uint8_t *cell_tables, int k, uint8_t *means, uint8_t *cnq,
                                const uint32_t *shared_idx, uint32_t n_shared, unsigned long long *shared,
                                gcn10_stream_t stream)
{
    const char *const who = "gcn10_gpu_grid_finish_rains";
    int rc = use_device(ctx);
    if (rc)
        return rc;
    hipStream_t s = as_stream(ctx, stream);
    if ((rc = check_rain_tables(ctx, who)) != GCN10_OK)
        return rc;
    if ((rc = check_layers(who, cell_tables, k)) != GCN10_OK)
        return rc;
    rc = check_finish_args(who, acc, n_sel, n_cells, means, shared_idx, n_shared, shared, cnq != nullptr);
    if (rc != GCN10_OK)
        return rc;
    RainsFinishParams p = {};
    p.acc = acc;
    p.n_cells = n_cells;
    p.means = means;
    p.cnq = cnq;
    p.shared_idx = shared_idx;
    p.n_shared = n_shared;
    p.shared = shared;
    p.cell_tables = cell_tables;
    p.tables = ctx->d_rain_tables;
    p.n_tables = (uint32_t)ctx->n_rain_tables;
    p.k = (uint32_t)k;
    p.n_sel = (uint32_t)n_sel;
    const size_t threads = n_cells > n_shared ? n_cells : n_shared;
    const uint32_t grid = (uint32_t)((threads + kFinishThreads - 1u) / kFinishThreads);
    hipLaunchKernelGGL(grid_finish_rains_kernel, dim3(grid, (uint32_t)n_sel), dim3(kFinishThreads), 0, s, p);
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}

}  // extern "C"
