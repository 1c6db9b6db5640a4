// gcn10_runoff_strip.hip -- gcn10_gpu_runoff_strip: the 18 rasters of a strip, every value sent through a byte table that
// is chosen PER CELL of a coarse grid (config key runoff_rain=..., DESIGN.md "Runoff rasters under a rainfall raster"):
//     out[r][y * W + x] = T[cell_table[celly[y] * ncx + cellx[x]]][v],    v = what gcn10_gpu_cn_strip writes there,
// and 255 where a map names no cell.  The library knows nothing about runoff: T is k tables of 256 bytes, applied as
// given (gcn10_gpu_set_cell_byte_tables).
//
// The kernel is cn_strip's code-bytes form with a second gather.  It moves the same bytes -- 1 B of landcover in, 18 B
// out per pixel, 16 B per lane and stream, nontemporal -- and reads one more L2-resident stream beside the soil bytes:
//   tix  [ncy + 1][stride]  uint16   the table of every (cell row, fine column): cell_table through cellx, an entry >= k
//                                    folded to 0, and k where cellx names no cell.  Row ncy is all k: the row of a strip
//                                    row that celly puts in no cell.  A pre-kernel of the call writes it
//                                    (expand_cell_tables_kernel) into a workspace of the context.
// In LDS, behind the 24 KiB all-tables image, lie the k tables and a table k of 256 bytes 255, so "in no cell" is a
// table like any other and the loop has no branch for it: a pixel costs one ds_read_b128 per condition (gather16) and
// one ds_read_u8 per raster at entry * 260 + v.  The entries are used pixel by pixel; nothing is assumed about the size
// or the order of the cells.
//
// The LDS of a workgroup is 24672 + (k + 1) * 260 bytes, dynamic, checked against the device.  With many tables (k = 256:
// 89.3 KiB, one workgroup per CU) the workgroup has 1024 threads, so that a CU still holds 16 waves; with k <= 32 it has
// 256 and four of them share a CU.  The grid is capped (gcn10::grid_cap) at the workgroups that are resident at once --
// the kernel's registers allow 4 waves per SIMD --, each looping over chunks of 16 px per thread in XCD slabs
// (first_chunk): a workgroup stages its tables once.
//
// Rows, columns and the straddling lane of W % 16 != 0 are those of issue_trip in gcn10_strip.hip; W < 1040, a
// misaligned pointer and the W * rows % 16 tail go pixel by pixel.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "gcn10_gpu.h"
#include "gcn10_device_util.hpp"
#include "gcn10_gpu_internal.hpp"
#include "gcn10_soil_readers.hpp"

using namespace gcn10;

namespace {

constexpr uint32_t kWavePx = 64u * kPxPerLane;          // 1024 px per wave and trip
constexpr uint32_t kMinVectorW = kWavePx + 16u;         // a wave's span crosses at most one row end
constexpr uint32_t kTixPad = 16u;                       // entries in front of row 0 and behind every row
constexpr int kSmallThreads = 256, kLargeThreads = 1024;
constexpr int kSmallTables = 32;                        // up to here a workgroup has kSmallThreads threads
constexpr int kSmallPerCu = 4, kLargePerCu = 1;         // workgroups per CU at the kernel's 4 waves per SIMD, LDS permitting
constexpr int kExpandThreads = 256;
// A table takes 260 bytes of LDS: with 256, the bank of T[t][v] would depend on v alone, and the lanes of a wave that hold
// the same value under different tables -- the common case where rain cells meet inside a wave's 1024 px -- would all
// fall on one bank.  With 65 dwords per table the table shifts the bank.
constexpr uint32_t kTableStride = 260u;

struct RunoffParams {
    const uint8_t *esa;
    SoilView soil;
    const uint8_t *lut;             // the all-tables image
    const uint8_t *tables;          // [k + 1][256]: the byte tables, then 256 bytes 255
    uint32_t n_tables;              // k + 1
    const uint16_t *tix;            // row 0 of the expanded tables
    uint32_t tix_stride;            // entries per row: W + kTixPad
    const int32_t *celly;
    uint32_t ncy;
    uint8_t *out[GCN10_N_RASTERS];
    uint32_t W, rows, npix;
    uint32_t nvec16;                // pixels done 16 per lane: npix rounded down, or 0 (all pixel by pixel)
    uint32_t nchunks;
    uint32_t cond_mask, table_mask;
};

struct ExpandParams {
    const int32_t *cellx;
    const uint8_t *cell_table;
    uint32_t ncx, ncy, k, W, stride;
    uint16_t *ws;                   // the workspace: kTixPad entries, then ncy + 1 rows
    uint64_t total;                 // kTixPad + (ncy + 1) * stride
};

// one thread per entry of the workspace, the padding included: nothing in it stays unwritten
__global__ __launch_bounds__(kExpandThreads) void expand_cell_tables_kernel(const ExpandParams p)
{
    const uint64_t i = (uint64_t)blockIdx.x * kExpandThreads + threadIdx.x;
    if (i >= p.total)
        return;
    uint32_t e = p.k;
    if (i >= kTixPad) {
        const uint64_t j = i - kTixPad;
        const uint32_t row = (uint32_t)(j / p.stride), x = (uint32_t)(j - (uint64_t)row * p.stride);
        if (row < p.ncy && x < p.W) {
            const uint32_t cx = (uint32_t)p.cellx[x];
            if (cx < p.ncx) {
                const uint32_t tb = p.cell_table[(size_t)row * p.ncx + cx];
                e = tb < p.k ? tb : 0u;
            }
        }
    }
    p.ws[i] = (uint16_t)e;
}

// the row of tix of a strip row: its cell row, or the all-k row
__device__ __forceinline__ uint32_t tix_row(const RunoffParams &p, int32_t cy)
{
    return (uint32_t)cy < p.ncy ? (uint32_t)cy : p.ncy;
}

// one pixel, every selected raster
__device__ __forceinline__ void runoff_pixel(const RunoffParams &p, const uint8_t *lut, const uint8_t *T, uint32_t i)
{
    const uint32_t y = i / p.W;
    const uint32_t x = i - y * p.W;
    const uint32_t lc = p.esa[i];
    const uint32_t cd = *p.soil.ptr(y, x);
    const uint32_t off = (uint32_t)p.tix[(size_t)tix_row(p, p.celly[y]) * p.tix_stride + x] * kTableStride;
    for (int c = 0; c < 2; c++) {
        if (!(p.cond_mask & (1u << c)))
            continue;
        const uint8_t *row = lut16_row(lut, (cd >> (4 * c)) & 0xfu, lc);
        for (int k = 0; k < 9; k++)
            if (p.table_mask & (1u << k))
                p.out[c * 9 + k][i] = T[off + row[k]];
    }
}

// bytes [0, 2n) of a lane's 32 bytes of entries from a, the rest from b (n = entries still in the lane's row)
__device__ __forceinline__ uint32_t entry_mask(uint32_t n, int j)
{
    const int32_t m = 2 * (int32_t)n - 4 * j;
    return m >= 4 ? 0xffffffffu : (m <= 0 ? 0u : 0xffffu);
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void runoff_strip_kernel(const RunoffParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t *const lut = lds;
    uint8_t *const T = lds + kLut16Bytes;

    stage_lut16<THREADS>(lut, p.lut);
    for (uint32_t i = threadIdx.x; i < p.n_tables * 64u; i += THREADS)      // dwords; 64 of a table, then one of padding
        reinterpret_cast<uint32_t *>(T)[(i >> 6) * (kTableStride / 4u) + (i & 63u)] =
            reinterpret_cast<const uint32_t *>(p.tables)[i];
    __syncthreads();

    if (p.nvec16 == 0u) {
        // any alignment, any shape
        const uint32_t stride = gridDim.x * THREADS;
        for (uint32_t i = blockIdx.x * THREADS + threadIdx.x; i < p.npix; i += stride)
            runoff_pixel(p, lut, T, i);
        return;
    }

    constexpr uint32_t kChunkPx = (uint32_t)THREADS * kPxPerLane;
    const uint32_t lane_off = (threadIdx.x & 63u) * kPxPerLane;
    const uint32_t wave_off = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * kWavePx;
    uint32_t step, end;
    for (uint32_t chunk = first_chunk(p.nchunks, step, end, true); chunk < end; chunk += step) {
        // ---- wave-uniform: row and column of the wave's first pixel; the soil rows and the cell rows of that strip
        // row and of the next one through the scalar cache ----
        const uint32_t wb = __builtin_amdgcn_readfirstlane(chunk * kChunkPx + wave_off);
        const uint32_t wbc = wb < p.npix ? wb : 0u;         // a wave past the end only needs valid addresses
        const uint32_t y = wbc / p.W;
        const uint32_t xb = wbc - y * p.W;
        const uint32_t y1 = y + 1u < p.rows ? y + 1u : y;
        const uint32_t r0 = (uint32_t)scalar_load_i32(p.soil.cj, y);
        const uint32_t r1 = (uint32_t)scalar_load_i32(p.soil.cj, y1);
        const uint32_t g0 = tix_row(p, scalar_load_i32(p.celly, y));
        const uint32_t g1 = tix_row(p, scalar_load_i32(p.celly, y1));

        const uint32_t i0 = wb + lane_off;
        const bool live = i0 < p.nvec16;
        const u32x4 e16 = load16_aligned_nt(p.esa + (live ? i0 : 0u));

        uint32_t xl = xb + lane_off;
        const bool wrap = xl >= p.W;
        xl = wrap ? xl - p.W : xl;
        const uint8_t *pa = p.soil.at(p.soil.clamp(wrap ? r1 : r0), xl);
        const uint16_t *ta = p.tix + (size_t)(wrap ? g1 : g0) * p.tix_stride + xl;
        u32x4 c16 = load16_any(pa);
        u32x4 t0 = load16_any(reinterpret_cast<const uint8_t *>(ta));
        u32x4 t1 = load16_any(reinterpret_cast<const uint8_t *>(ta + 8));
        if (p.W & 15u) {
            const uint32_t n = p.W - xl;                    // pixels of this lane that are still in its row
            const bool strad = !wrap && n < (uint32_t)kPxPerLane;
            if (__builtin_amdgcn_ballot_w64(strad) != 0ull) {
                // the other lanes of this wave re-read their own vectors (L1 hits)
                const uint8_t *pb = strad ? p.soil.at(p.soil.clamp(r1), 0u) - n : pa;
                const uint16_t *tb = strad ? p.tix + (size_t)g1 * p.tix_stride - n : ta;
                const u32x4 b = load16_any(pb);
                const u32x4 b0 = load16_any(reinterpret_cast<const uint8_t *>(tb));
                const u32x4 b1 = load16_any(reinterpret_cast<const uint8_t *>(tb + 8));
                const uint32_t nn = strad ? n : (uint32_t)kPxPerLane;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int32_t m = (int32_t)nn - 4 * j;
                    const uint32_t mask = m >= 4 ? 0xffffffffu : (m <= 0 ? 0u : (1u << (8 * m)) - 1u);
                    c16[j] = (c16[j] & mask) | (b[j] & ~mask);
                    const uint32_t m0 = entry_mask(nn, j), m1 = entry_mask(nn, j + 4);
                    t0[j] = (t0[j] & m0) | (b0[j] & ~m0);
                    t1[j] = (t1[j] & m1) | (b1[j] & ~m1);
                }
            }
        }

        // the table of every pixel as an offset into T
        uint32_t off[16];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            off[2 * j] = (t0[j] & 0xffffu) * kTableStride;
            off[2 * j + 1] = (t0[j] >> 16) * kTableStride;
            off[8 + 2 * j] = (t1[j] & 0xffffu) * kTableStride;
            off[8 + 2 * j + 1] = (t1[j] >> 16) * kTableStride;
        }

#pragma unroll
        for (int c = 0; c < 2; c++) {
            if (!(p.cond_mask & (1u << c)))
                continue;
            uint32_t acc[9][4];
            gather16(lut, e16, c16, c, acc);
#pragma unroll
            for (int k = 0; k < 9; k++) {
                if (!(p.table_mask & (1u << k)))
                    continue;
                u32x4 v;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint32_t a = acc[k][j];
                    const uint32_t q0 = T[off[4 * j] + (a & 0xffu)];
                    const uint32_t q1 = T[off[4 * j + 1] + ((a >> 8) & 0xffu)];
                    const uint32_t q2 = T[off[4 * j + 2] + ((a >> 16) & 0xffu)];
                    const uint32_t q3 = T[off[4 * j + 3] + (a >> 24)];
                    v[j] = q0 | q1 << 8 | q2 << 16 | q3 << 24;
                }
                if (live)
                    store16<true>(p.out[c * 9 + k] + i0, v);
            }
        }
    }

    // the last npix % 16 pixels, one per thread
    if (blockIdx.x == 0 && threadIdx.x < p.npix - p.nvec16)
        runoff_pixel(p, lut, T, p.nvec16 + threadIdx.x);
}

// as gcn10::launch_timed, for a workgroup of `threads` threads with dynamic LDS
hipError_t launch(gcn10_gpu_ctx *ctx, const void *fn, uint32_t grid, int threads, size_t lds, void **args, hipStream_t s)
{
    if (!ctx->time_start || !ctx->time_stop)
        return hipLaunchKernel(fn, dim3(grid), dim3(threads), args, lds, s);
    const hipError_t e = hipExtLaunchKernel(fn, dim3(grid), dim3(threads), args, lds, s, ctx->time_start,
                                            ctx->time_stop, 0);
    if (e == hipSuccess)
        ctx->time_start = ctx->time_stop = nullptr;
    return e;
}

}  // namespace

extern "C" {

int gcn10_gpu_set_cell_byte_tables(gcn10_gpu_ctx *ctx, const uint8_t *t, int k)
{
    const char *const who = "gcn10_gpu_set_cell_byte_tables";
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (!t || k < 1 || k > GCN10_GPU_MAX_CELL_BYTE_TABLES)
        return fail(GCN10_E_INVAL, "%s: bad arguments k=%d (1..%d tables, no null bytes)", who, k,
                    GCN10_GPU_MAX_CELL_BYTE_TABLES);
    ctx->n_cell_byte_tables = 0;
    if (!ctx->d_cell_byte_tables)       // once, for the most tables a context takes and the table of "no cell"
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ctx->d_cell_byte_tables),
                          (GCN10_GPU_MAX_CELL_BYTE_TABLES + 1) * 256));
    // synchronous: once per run, read by every later call on any stream
    HIP_TRY(hipDeviceSynchronize());    // an earlier strip may still read the tables
    HIP_TRY(hipMemcpy(ctx->d_cell_byte_tables, t, (size_t)k * 256, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(ctx->d_cell_byte_tables + (size_t)k * 256, 255, 256));
    HIP_TRY(hipDeviceSynchronize());
    ctx->n_cell_byte_tables = k;
    return GCN10_OK;
}

int gcn10_gpu_runoff_strip(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                           const int32_t *cellx_dev, const int32_t *celly_dev, int ncx, int ncy,
                           const uint8_t *cell_table_dev, unsigned cond_mask, unsigned table_mask,
                           uint8_t *const out[GCN10_N_RASTERS], gcn10_stream_t stream)
{
    const char *const who = "gcn10_gpu_runoff_strip";
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if ((rc = check_tables(ctx, who)) != GCN10_OK || (rc = check_tile(ctx, who)) != GCN10_OK)
        return rc;
    if (ctx->n_cell_byte_tables <= 0)
        return fail(GCN10_E_STATE, "%s: call gcn10_gpu_set_cell_byte_tables first", who);
    if (W <= 0 || rows <= 0 || ncx <= 0 || ncy <= 0)
        return fail(GCN10_E_INVAL, "%s: bad shape W=%d rows=%d ncx=%d ncy=%d", who, W, rows, ncx, ncy);
    if ((uint64_t)W * (uint64_t)rows > 0x7fffffffull)
        return fail(GCN10_E_INVAL, "%s: strip of %d x %d exceeds 2^31-1 pixels", who, W, rows);
    if ((rc = check_masks(ctx, who, cond_mask, table_mask)) != GCN10_OK)
        return rc;
    if (!esa || !cj || !cellx_dev || !celly_dev || !cell_table_dev || !out)
        return fail(GCN10_E_INVAL, "%s: null pointer", who);

    RunoffParams p;
    memset(&p, 0, sizeof p);
    bool all_aligned = aligned16(esa);
    for (int r = 0; r < GCN10_N_RASTERS; r++) {
        if (!selected(r, cond_mask, table_mask))
            continue;
        if (!out[r])
            return fail(GCN10_E_INVAL, "%s: out[%d] is null but selected", who, r);
        p.out[r] = out[r];
        all_aligned = all_aligned && aligned16(out[r]);
    }
    hipStream_t s = as_stream(ctx, stream);
    if ((rc = bind_soil(ctx, who, W, s, cj, &p.soil)) != GCN10_OK)
        return rc;

    // the LDS of a workgroup and of a CU, from the device
    const int k = ctx->n_cell_byte_tables;
    const size_t lds = (size_t)kLut16Bytes + ((size_t)k + 1u) * kTableStride;
    int lds_wg = 0, lds_cu = 0;
    HIP_TRY(hipDeviceGetAttribute(&lds_wg, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
    HIP_TRY(hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, ctx->device));
    if ((size_t)lds_wg < lds)
        return fail(GCN10_E_STATE, "%s: the device gives a workgroup %d bytes of LDS, %d tables take %zu", who, lds_wg, k,
                    lds);
    lds_cu = lds_cu < lds_wg ? lds_wg : lds_cu;
    if (!ctx->runoff_strip_ready) {
        const int most = kLut16Bytes + (GCN10_GPU_MAX_CELL_BYTE_TABLES + 1) * (int)kTableStride;
        const int ask = most < lds_wg ? most : lds_wg;
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(runoff_strip_kernel<kSmallThreads>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, ask));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(runoff_strip_kernel<kLargeThreads>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, ask));
        ctx->runoff_strip_ready = true;
    }

    // the table of every (cell row, fine column)
    ExpandParams x;
    memset(&x, 0, sizeof x);
    x.stride = (uint32_t)W + kTixPad;
    x.total = (uint64_t)kTixPad + ((uint64_t)ncy + 1u) * x.stride;
    const uint64_t xgrid = (x.total + kExpandThreads - 1u) / kExpandThreads;
    if (xgrid > 0x7fffffffull)
        return fail(GCN10_E_INVAL, "%s: %d cell rows x %d columns: cut the cell rectangle", who, ncy, W);
    if ((rc = grow_workspace(&ctx->ws.cell_tables, &ctx->ws.cell_tables_cap, x.total * sizeof(uint16_t))) != GCN10_OK)
        return rc;
    x.cellx = cellx_dev;
    x.cell_table = cell_table_dev;
    x.ncx = (uint32_t)ncx;
    x.ncy = (uint32_t)ncy;
    x.k = (uint32_t)k;
    x.W = (uint32_t)W;
    x.ws = static_cast<uint16_t *>(ctx->ws.cell_tables);
    hipLaunchKernelGGL(expand_cell_tables_kernel, dim3((uint32_t)xgrid), dim3(kExpandThreads), 0, s, x);
    HIP_TRY(hipGetLastError());

    p.esa = esa;
    p.lut = ctx->d_lut16;
    p.tables = ctx->d_cell_byte_tables;
    p.n_tables = (uint32_t)k + 1u;
    p.tix = x.ws + kTixPad;
    p.tix_stride = x.stride;
    p.celly = celly_dev;
    p.ncy = (uint32_t)ncy;
    p.W = (uint32_t)W;
    p.rows = (uint32_t)rows;
    p.npix = (uint32_t)((uint64_t)W * (uint64_t)rows);
    p.cond_mask = cond_mask;
    p.table_mask = table_mask;
    // the vector path wants a wave's 1024-px span to cross at most one row end
    if (p.npix < 16u || p.W < kMinVectorW)
        all_aligned = false;
    p.nvec16 = all_aligned ? p.npix & ~15u : 0u;

    const bool large = k > kSmallTables;
    const int threads = large ? kLargeThreads : kSmallThreads;
    const uint32_t unit = all_aligned ? (uint32_t)threads * kPxPerLane : (uint32_t)threads;
    p.nchunks = (uint32_t)(((uint64_t)p.npix + unit - 1u) / unit);
    int per_cu = (int)((size_t)lds_cu / lds);
    per_cu = per_cu < 1 ? 1 : (per_cu > (large ? kLargePerCu : kSmallPerCu) ? (large ? kLargePerCu : kSmallPerCu) : per_cu);
    uint32_t cap = grid_cap(ctx, per_cu);
    cap -= cap % 8u;                    // every XCD the same number of workgroups
    cap = cap < 8u ? 8u : cap;
    const uint32_t grid = p.nchunks < cap ? p.nchunks : cap;
    const void *fn = large ? reinterpret_cast<const void *>(runoff_strip_kernel<kLargeThreads>)
                           : reinterpret_cast<const void *>(runoff_strip_kernel<kSmallThreads>);
    void *args[] = { &p };
    HIP_TRY(launch(ctx, fn, grid, threads, lds, args, s));
    ctx->last_kernel = large ? "runoff_strip_kernel<1024>" : "runoff_strip_kernel<256>";
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}

}  // extern "C"
