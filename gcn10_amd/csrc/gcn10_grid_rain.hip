// gcn10_grid_rain.hip -- the triples {s, n, sw} of every selected raster over the cells of a model grid, with the weight
// table chosen PER CELL (config key rain=..., DESIGN.md "Rainfall raster").
//
// gcn10_grid.hip folds one weight table into image planes, which ties a table to a whole launch.  Here a cell's
// triples come from its (landcover, soil code) pair histogram instead: every raster's value at a pixel is a function
// of the pixel's pair (gcn10_stats.hip), so the histogram of a cell gives s, n and the sum of w[v] for all 18 rasters
// and for any table w, in integers.
//
// The unit of work is an item: kItemCols columns x at most kItemRows rows of the strip, 65024 pixels at most, so that
// a count fits 16 bits and every 32-bit sum of an item holds (65024 x 65535 < 2^32).  A WAVE owns an item -- a
// workgroup is one wave, its LDS the 4096-word histogram of pair_histogram_kernel -- and walks the pieces of cells in
// it: the runs of equal entries of celly in its rows, and within each the runs of equal entries of cellx in its
// columns, found with a ballot over 64 entries at a time.  A run whose value is no cell is stepped over; a cell that
// the maps name in two runs is two pieces that add to the same words, so the sums are right for ANY maps, and a cell
// index is tested against ncx / ncy before it is used.  There is no LDS image of cell columns and no limit on how many
// an item meets.
//
// A piece is counted in (row, 16-column group) units dealt to the 64 lanes, so a piece of 25 x 25 pixels keeps every
// lane busy: a whole group goes through count16, one that a piece edge cuts through count_masked, the row's last group
// with W % 16 != 0 through count_tail (nothing at or beyond W is read).  Then the non-zero bins are packed in place to
// the front of the histogram (bin << 16 | count; the words read are cleared on the way), a lane takes packed bins and
// looks the value of every selected raster up in the all-tables image in global memory (lut16_row: a few dozen rows
// per piece) and the weight in the cell's own 512-byte table, and the lanes' 54 partial sums are transposed through
// the now empty histogram so that lane j adds up word j: ONE 64-bit atomic add per (raster, word) of the piece.  ADD
// semantics leave no place for plain stores: acc is never known to be zero.
//
// The launch is not capped: one workgroup per item.  gcn10_gpu_grid_finish_rain is one thread per (raster, cell).
//
// The item, the walk of the pieces, the counting and the pack are in gcn10_grid_rain_piece.hpp, which
// gcn10_grid_rains.hip (k tables per cell) uses too; what follows the pack is this file's own.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "gcn10_grid_internal.hpp"
#include "gcn10_grid_rain_piece.hpp"

using namespace gcn10;
using namespace gcn10::rain_piece;

namespace {

constexpr uint32_t kSums = 2u * 9u * 3u;                    // partial sums of a lane: (condition, table, word)
constexpr uint32_t kSumStride = kSums + 1u;                 // odd: the lanes' sums fall in different LDS banks
constexpr int kFinishThreads = 256;
static_assert(kSumStride * kWave <= (uint32_t)kHistWords, "the transpose fits the histogram");

struct RainParams {
    const uint8_t *esa;             // strip, W x rows, row major
    SoilView soil;                  // soil code bytes, soil row of every strip row
    const uint8_t *lut;             // the all-tables image, in global memory
    const int32_t *cellx, *celly;
    const uint8_t *cell_table;      // [ncy][ncx]: the table of every cell
    const uint16_t *tables;         // [n_tables][256]
    uint32_t n_tables;
    uint32_t W, rows, ncx, ncy;
    uint32_t chunks, band_rows;
    uint32_t sel;                   // bit r: raster r is selected
    uint32_t n_conds, conds[2];     // the selected conditions
    unsigned long long *acc;        // [n_sel][ncy][ncx][3]
};

// Columns [xa, xb) x rows [ya, yb) of cell (cx, cy), all inside the wave's item: counted, reduced against the cell's
// table and added to the cell's triples.  h is all zero before and after.
__device__ __forceinline__ void sum_piece(const RainParams &p, uint32_t *h, uint32_t xa, uint32_t xb, uint32_t ya,
                                          uint32_t yb, uint32_t cx, uint32_t cy)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t m = count_and_pack(p, h, xa, xb, ya, yb);
    if (m == 0u)
        return;                 // the same for the whole wave

    // a lane's packed bins against the image and the cell's table
    const size_t cell = (size_t)cy * p.ncx + cx;
    const uint32_t tb = p.cell_table[cell];
    const uint16_t *const w = p.tables + 256u * (tb < p.n_tables ? tb : 0u);
    uint32_t sum[2][9][3];
#pragma unroll
    for (uint32_t ci = 0; ci < 2; ci++)
#pragma unroll
        for (uint32_t t = 0; t < 9; t++)
            sum[ci][t][0] = sum[ci][t][1] = sum[ci][t][2] = 0u;
    for (uint32_t i = lane; i < m; i += kWave) {
        const uint32_t ent = h[i];
        h[i] = 0u;
        const uint32_t c = ent & 0xffffu, lc = (ent >> 16) & 255u, code = bin_code(ent >> 24);
#pragma unroll
        for (uint32_t ci = 0; ci < 2; ci++) {
            if (ci >= p.n_conds)
                continue;
            const uint32_t cond = p.conds[ci], sel9 = (p.sel >> (9u * cond)) & 0x1ffu;
            const uint8_t *const row = lut16_row(p.lut, (code >> (4u * cond)) & 15u, lc);
            const u32x4 r = *reinterpret_cast<const u32x4 *>(row);
#pragma unroll
            for (uint32_t t = 0; t < 9; t++) {
                const uint32_t v = (r[t >> 2] >> (8u * (t & 3u))) & 255u;
                if ((sel9 >> t) & 1u && v != GCN10_NODATA) {
                    sum[ci][t][0] += c * v;
                    sum[ci][t][1] += c;
                    sum[ci][t][2] += c * w[v];
                }
            }
        }
    }
    __syncthreads();

    // transposed through the empty histogram, kSumStride words per lane that had bins: lane j adds up sum j of all
    const uint32_t nl = min(m, kWave);
    if (lane < nl) {
#pragma unroll
        for (uint32_t ci = 0; ci < 2; ci++)
#pragma unroll
            for (uint32_t t = 0; t < 9; t++)
#pragma unroll
                for (uint32_t word = 0; word < 3; word++)
                    h[lane * kSumStride + (ci * 9u + t) * 3u + word] = sum[ci][t][word];
    }
    __syncthreads();
    uint32_t total = 0u;
    if (lane < kSums)
        for (uint32_t l = 0; l < nl; l++)
            total += h[l * kSumStride + lane];
    __syncthreads();
    if (lane < nl) {
#pragma unroll
        for (uint32_t j = 0; j < kSums; j++)
            h[lane * kSumStride + j] = 0u;
    }
    __syncthreads();
    if (lane < kSums && total) {
        const uint32_t ci = lane / 27u, t = (lane - 27u * ci) / 3u, word = lane % 3u;
        const uint32_t r = 9u * p.conds[ci] + t;            // sums of a condition that is not selected are zero
        const uint32_t q = __popc(p.sel & ((1u << r) - 1u));
        atomicAdd(p.acc + ((size_t)q * p.ncy * p.ncx + cell) * 3u + word, (unsigned long long)total);
    }
}

__global__ __launch_bounds__(kWave) void grid_sums_rain_kernel(const RainParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t h[kHistWords];
    walk_item(p, h, [&](uint32_t xa, uint32_t xb, uint32_t ya, uint32_t yb, uint32_t cx, uint32_t cy) {
        sum_piece(p, h, xa, xb, ya, yb, cx, cy);
    });
}

struct RainFinishParams {
    const unsigned long long *acc;
    size_t n_cells;
    uint8_t *means, *cnq;
    const uint32_t *shared_idx;
    uint32_t n_shared;
    unsigned long long *shared;
    const uint8_t *cell_table;
    const uint16_t *tables;         // [n_tables][256], then a byte per table: entries 1..100 never decrease
    uint32_t n_tables;
};

// blockIdx.y: the raster; a thread: a cell, and a shared cell
__global__ __launch_bounds__(kFinishThreads) void grid_finish_rain_kernel(const RainFinishParams p)
{
    const size_t q = blockIdx.y, i = (size_t)blockIdx.x * kFinishThreads + threadIdx.x;
    if (i < p.n_cells) {
        const unsigned long long *const a = p.acc + 3u * (q * p.n_cells + i);
        const unsigned long long s = a[0], n = a[1], sw = a[2];
        const uint32_t tb = p.cell_table[i], t = tb < p.n_tables ? tb : 0u;
        const uint8_t *const rising = reinterpret_cast<const uint8_t *>(p.tables + 256u * p.n_tables);
        p.means[q * p.n_cells + i] = mean_byte(s, n);
        p.cnq[q * p.n_cells + i] = runoff_cn(p.tables + 256u * t, rising[t] != 0, s, n, sw);
    }
    if (i < p.n_shared) {
        const unsigned long long *const a = p.acc + 3u * (q * p.n_cells + p.shared_idx[i]);
        unsigned long long *const to = p.shared + 3u * (q * p.n_shared + i);
        to[0] = a[0];
        to[1] = a[1];
        to[2] = a[2];
    }
}

}  // namespace

extern "C" {

int gcn10_gpu_grid_rain_item(int *cols, int *rows)
{
    if (cols)
        *cols = (int)kItemCols;
    if (rows)
        *rows = (int)kItemRows;
    return (int)(kItemCols * kItemRows);
}

int gcn10_gpu_set_rain_tables(gcn10_gpu_ctx *ctx, const uint16_t *w, int k)
{
    const char *const who = "gcn10_gpu_set_rain_tables";
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (!w || k < 1 || k > GCN10_GPU_MAX_RAIN_TABLES)
        return fail(GCN10_E_INVAL, "%s: bad arguments k=%d (1..%d tables, no null weights)", who, k,
                    GCN10_GPU_MAX_RAIN_TABLES);
    // the tables, then the "never decreases over 1..100" byte of each
    const size_t table_bytes = 256 * sizeof(uint16_t);
    uint8_t rising[GCN10_GPU_MAX_RAIN_TABLES];
    for (int j = 0; j < k; j++)
        rising[j] = never_decreases(w + 256 * j);
    ctx->n_rain_tables = 0;
    if (!ctx->d_rain_tables)            // once, for the most tables a context takes
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ctx->d_rain_tables),
                          GCN10_GPU_MAX_RAIN_TABLES * (table_bytes + 1)));
    // synchronous: once per run, read by every later rain call on any stream
    HIP_TRY(hipMemcpy(ctx->d_rain_tables, w, (size_t)k * table_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(reinterpret_cast<uint8_t *>(ctx->d_rain_tables) + (size_t)k * table_bytes, rising, (size_t)k,
                      hipMemcpyHostToDevice));
    ctx->n_rain_tables = k;
    return GCN10_OK;
}

int gcn10_gpu_grid_sums_rain(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                             const int32_t *cellx, const int32_t *celly, int ncx, int ncy, unsigned cond_mask,
                             unsigned table_mask, const uint8_t *cell_table, unsigned long long *acc,
                             gcn10_stream_t stream)
{
    const char *const who = "gcn10_gpu_grid_sums_rain";
    int rc = use_device(ctx);
    if (rc)
        return rc;
    hipStream_t s = as_stream(ctx, stream);
    RainParams p = {};
    if ((rc = check_tables(ctx, who)) != GCN10_OK)
        return rc;
    if ((rc = check_rain_tables(ctx, who)) != GCN10_OK)
        return rc;
    if ((rc = bind_soil(ctx, who, W, s, cj, &p.soil)) != GCN10_OK)
        return rc;
    if ((rc = check_sums_args(who, esa, W, rows, cj, cellx, celly, ncx, ncy, acc, cell_table != nullptr)) != GCN10_OK)
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
    p.cell_table = cell_table;
    p.tables = ctx->d_rain_tables;
    p.n_tables = (uint32_t)ctx->n_rain_tables;
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
    hipLaunchKernelGGL(grid_sums_rain_kernel, dim3((uint32_t)grid), dim3(kWave), 0, s, p);
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}

int gcn10_gpu_grid_finish_rain(gcn10_gpu_ctx *ctx, const unsigned long long *acc, int n_sel, size_t n_cells,
                               const uint8_t *cell_table, uint8_t *means, uint8_t *cnq, const uint32_t *shared_idx,
                               uint32_t n_shared, unsigned long long *shared, gcn10_stream_t stream)
{
    const char *const who = "gcn10_gpu_grid_finish_rain";
    int rc = use_device(ctx);
    if (rc)
        return rc;
    hipStream_t s = as_stream(ctx, stream);
    if ((rc = check_rain_tables(ctx, who)) != GCN10_OK)
        return rc;
    rc = check_finish_args(who, acc, n_sel, n_cells, means, shared_idx, n_shared, shared, cell_table && cnq);
    if (rc != GCN10_OK)
        return rc;
    RainFinishParams p = {};
    p.acc = acc;
    p.n_cells = n_cells;
    p.means = means;
    p.cnq = cnq;
    p.shared_idx = shared_idx;
    p.n_shared = n_shared;
    p.shared = shared;
    p.cell_table = cell_table;
    p.tables = ctx->d_rain_tables;
    p.n_tables = (uint32_t)ctx->n_rain_tables;
    const size_t threads = n_cells > n_shared ? n_cells : n_shared;
    const uint32_t grid = (uint32_t)((threads + kFinishThreads - 1u) / kFinishThreads);
    hipLaunchKernelGGL(grid_finish_rain_kernel, dim3(grid, (uint32_t)n_sel), dim3(kFinishThreads), 0, s, p);
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}

}  // extern "C"
