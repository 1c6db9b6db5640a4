// gcn10_verify.hip -- compares decoded CN rasters with the values computed now (config key verify=1, DESIGN.md
// "Verification").
//
// gcn10_gpu_verify_strip: one pass over a landcover strip.  Every lane takes 16 consecutive pixels of one row, forms
// their soil codes and the up to 18 table values with the all-tables strip kernel's own gather -- gcn10::gather16 of
// gcn10_soil_readers.hpp over the same LDS image, which finish_trip of gcn10_strip.hip calls too (one 16-byte LDS row
// per pixel and drainage condition, 4x4 byte transposes) -- and XORs them with the 16 bytes of each selected file
// raster.  The kernel only loads: 19 bytes per pixel with all rasters selected, all of a lane's loads issued before
// the first is used.  The expected rasters never exist in memory.
//
// Counting.  Differences are rare, so the common path of a raster is one OR over four dwords and one wave vote.
// A wave that holds a difference sums its lanes' counts and takes the minimum of their (y << 32 | x) keys with
// shuffles; one lane adds that to the workgroup's counters in LDS.  A workgroup touches the device counters once
// per raster when it ends, and only for rasters in which it found something.  `first` is a 64-bit minimum over
// block coordinates, so it depends on nothing but the pixels.  `want` / `got` of that pixel are written by a second
// launch of one small workgroup that recomputes the one pixel `first` names when it lies in the strip just checked
// (a pair of independent atomics could leave values of two different pixels).  Hence the rule in gcn10_gpu.h: the
// strips that add to one counts_dev are issued in stream order.
//
// Rows are addressed by (row, 16-pixel group), not as a flat array, because a decode buffer's rows are got_stride
// bytes apart.  The W % 16 pixels at each row's end are checked one pixel per lane after the vector part.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "gcn10_gpu_internal.hpp"
#include "gcn10_soil_readers.hpp"

using namespace gcn10;

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kPxPerLane = 16;
// workgroups per CU at most: the table is 24 KiB of LDS per workgroup and a lane holds 20 vectors
constexpr int kGridPerCu = 4;

struct VerifyParams {
    const uint8_t *esa;                     // strip, W x rows, row major                 (strip form)
    SoilView soil;                          // x-expanded soil codes, soil row of every strip row (strip form)
    const uint8_t *lut;                     // device image of the 16-byte-row table      (strip form)
    const uint8_t *want[GCN10_N_RASTERS];   // expected rasters                           (buffer form)
    const uint8_t *got[GCN10_N_RASTERS];
    gcn10_verify_count *counts;
    uint64_t want_stride, got_stride;
    uint32_t W, rows, y0;
    uint32_t groups_per_row;                // W / 16
    uint32_t n_groups;                      // rows * groups_per_row
    uint32_t sel;                           // bit r: raster r is compared
};

typedef u32x4 u32x4_u __attribute__((aligned(1)));

__device__ __forceinline__ u32x4 load16(const uint8_t *p)
{
    return *reinterpret_cast<const u32x4_u *>(p);
}

// read-once data (the file rasters): past the caches' keep lists
__device__ __forceinline__ u32x4 load16_once(const uint8_t *p)
{
    return __builtin_nontemporal_load(reinterpret_cast<const u32x4_u *>(p));
}

// 0x80 in every byte of d that is not zero
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t d)
{
    return (((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d) & 0x80808080u;
}

struct Tally {
    unsigned long long count[GCN10_N_RASTERS];
    unsigned long long first[GCN10_N_RASTERS];
};

__device__ __forceinline__ void tally_clear(Tally &t)
{
    if (threadIdx.x < GCN10_N_RASTERS) {
        t.count[threadIdx.x] = 0ull;
        t.first[threadIdx.x] = ~0ull;
    }
    __syncthreads();
}

// one device atomic per raster and workgroup for the count (and one for the minimum), none where nothing differed
__device__ __forceinline__ void tally_flush(Tally &t, gcn10_verify_count *counts)
{
    __syncthreads();
    if (threadIdx.x < GCN10_N_RASTERS && t.count[threadIdx.x]) {
        atomicAdd(reinterpret_cast<unsigned long long *>(&counts[threadIdx.x].mismatches), t.count[threadIdx.x]);
        atomicMin(reinterpret_cast<unsigned long long *>(&counts[threadIdx.x].first), t.first[threadIdx.x]);
    }
}

// The differing bytes of one raster in a wave: d = want ^ got of every lane's 16 pixels (all zero in lanes that
// have nothing to say), the lane's pixels start at (x, y) in block coordinates.  Called by whole waves.
__device__ __forceinline__ void tally_wave(Tally &t, int r, const uint32_t d[4], uint32_t x, uint32_t y)
{
    uint32_t n = 0u, at = 16u;
#pragma unroll
    for (int j = 3; j >= 0; j--) {
        const uint32_t m = nonzero_bytes(d[j]);
        n += (uint32_t)__popc(m);
        if (m)
            at = 4u * (uint32_t)j + (((uint32_t)__ffs((int)m) - 1u) >> 3);
    }
    unsigned long long key = n ? ((unsigned long long)y << 32) | (x + at) : ~0ull;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        n += (uint32_t)__shfl_xor((int)n, off);
        const unsigned long long other = (unsigned long long)__shfl_xor((long long)key, off);
        key = other < key ? other : key;
    }
    if ((threadIdx.x & 63u) == 0u) {
        atomicAdd(&t.count[r], (unsigned long long)n);
        atomicMin(&t.first[r], key);
    }
}

template <int C, bool ALL>
__device__ __forceinline__ void compare_cond(const VerifyParams &p, Tally &t, const uint8_t *lut, const u32x4 &e,
                                             const u32x4 &s, const u32x4 *g, bool live, uint32_t x, uint32_t y)
{
    if (!ALL && !((p.sel >> (9 * C)) & 0x1ffu))
        return;
    uint32_t acc[9][4];
    gather16(lut, e, s, C, acc);
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const int r = C * 9 + k;
        if (!ALL && !(p.sel & (1u << r)))
            continue;
        uint32_t d[4];
#pragma unroll
        for (int j = 0; j < 4; j++)
            d[j] = live ? acc[k][j] ^ g[r][j] : 0u;
        if (__any((d[0] | d[1] | d[2] | d[3]) != 0u))
            tally_wave(t, r, d, x, y);
    }
}

// ALL: all 18 rasters selected (no mask tests around the loads)
template <bool ALL>
__global__ __launch_bounds__(kThreads) void verify_strip_kernel(const VerifyParams p)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[kLut16Bytes];
    __shared__ Tally tally;
    stage_lut16<kThreads>(lut, p.lut);
    tally_clear(tally);

    // the trip count is the same for every lane of the workgroup, so whole waves reach the votes and shuffles
    const uint32_t trips = (p.n_groups + kThreads - 1u) / kThreads;
    for (uint32_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        const uint32_t gi = trip * kThreads + threadIdx.x;
        const bool live = gi < p.n_groups;
        const uint32_t gic = live ? gi : 0u;            // a lane past the end only needs valid addresses
        const uint32_t y = gic / p.groups_per_row;
        const uint32_t x = (gic - y * p.groups_per_row) * kPxPerLane;
        const u32x4 e = load16(p.esa + (size_t)y * p.W + x);
        const u32x4 s = *reinterpret_cast<const u32x4 *>(p.soil.ptr(y, x));
        u32x4 g[GCN10_N_RASTERS];
#pragma unroll
        for (int r = 0; r < GCN10_N_RASTERS; r++)
            if (ALL || (p.sel & (1u << r)))
                g[r] = load16_once(p.got[r] + (size_t)y * p.got_stride + x);
        compare_cond<0, ALL>(p, tally, lut, e, s, g, live, x, p.y0 + y);
        compare_cond<1, ALL>(p, tally, lut, e, s, g, live, x, p.y0 + y);
    }

    // the W % 16 pixels at the end of every row, one per lane
    const uint32_t tail = p.W - p.groups_per_row * kPxPerLane;
    const uint32_t n_tail = tail * p.rows;
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < n_tail; i += gridDim.x * kThreads) {
        const uint32_t y = i / tail;
        const uint32_t x = p.W - tail + (i - y * tail);
        const uint32_t lc = p.esa[(size_t)y * p.W + x];
        const uint32_t cd = *p.soil.ptr(y, x);
        for (int r = 0; r < GCN10_N_RASTERS; r++) {
            if (!(p.sel & (1u << r)))
                continue;
            const uint32_t plane = (cd >> (r >= 9 ? 4 : 0)) & 0xfu;
            const uint32_t want = lut16_value(lut, plane, lc, (uint32_t)(r % 9));
            if (want != p.got[r][(size_t)y * p.got_stride + x]) {
                atomicAdd(&tally.count[r], 1ull);
                atomicMin(&tally.first[r], ((unsigned long long)(p.y0 + y) << 32) | x);
            }
        }
    }
    tally_flush(tally, p.counts);
}

// expected rasters from memory: raster after raster, 16 pixels of each per lane
__global__ __launch_bounds__(kThreads) void verify_buffers_kernel(const VerifyParams p)
{
    __shared__ Tally tally;
    tally_clear(tally);

    const uint32_t trips = (p.n_groups + kThreads - 1u) / kThreads;
    for (uint32_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        const uint32_t gi = trip * kThreads + threadIdx.x;
        const bool live = gi < p.n_groups;
        const uint32_t gic = live ? gi : 0u;
        const uint32_t y = gic / p.groups_per_row;
        const uint32_t x = (gic - y * p.groups_per_row) * kPxPerLane;
        for (int r0 = 0; r0 < GCN10_N_RASTERS; r0 += 3) {
            if (!((p.sel >> r0) & 7u))
                continue;
            u32x4 w[3], g[3];
#pragma unroll
            for (int i = 0; i < 3; i++) {
                if (p.sel & (1u << (r0 + i))) {
                    w[i] = load16_once(p.want[r0 + i] + (size_t)y * p.want_stride + x);
                    g[i] = load16_once(p.got[r0 + i] + (size_t)y * p.got_stride + x);
                }
            }
#pragma unroll
            for (int i = 0; i < 3; i++) {
                if (!(p.sel & (1u << (r0 + i))))
                    continue;
                uint32_t d[4];
#pragma unroll
                for (int j = 0; j < 4; j++)
                    d[j] = live ? w[i][j] ^ g[i][j] : 0u;
                if (__any((d[0] | d[1] | d[2] | d[3]) != 0u))
                    tally_wave(tally, r0 + i, d, x, p.y0 + y);
            }
        }
    }

    const uint32_t tail = p.W - p.groups_per_row * kPxPerLane;
    const uint32_t n_tail = tail * p.rows;
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < n_tail; i += gridDim.x * kThreads) {
        const uint32_t y = i / tail;
        const uint32_t x = p.W - tail + (i - y * tail);
        for (int r = 0; r < GCN10_N_RASTERS; r++) {
            if (!(p.sel & (1u << r)))
                continue;
            if (p.want[r][(size_t)y * p.want_stride + x] != p.got[r][(size_t)y * p.got_stride + x]) {
                atomicAdd(&tally.count[r], 1ull);
                atomicMin(&tally.first[r], ((unsigned long long)(p.y0 + y) << 32) | x);
            }
        }
    }
    tally_flush(tally, p.counts);
}

// want / got of the pixel `first` names, when it lies in the rows just compared (one lane per raster)
template <bool FROM_TABLES>
__global__ void verify_first_kernel(const VerifyParams p)
{
    const uint32_t r = threadIdx.x;
    if (r >= GCN10_N_RASTERS || !(p.sel & (1u << r)))
        return;
    const uint64_t first = p.counts[r].first;
    const uint64_t y = first >> 32, x = first & 0xffffffffull;
    if (first == UINT64_MAX || y < p.y0 || y >= (uint64_t)p.y0 + p.rows || x >= p.W)
        return;
    const uint32_t ys = (uint32_t)(y - p.y0);
    uint32_t want;
    if (FROM_TABLES) {
        const uint32_t lc = p.esa[(size_t)ys * p.W + x];
        const uint32_t cd = *p.soil.ptr(ys, (uint32_t)x);
        const uint32_t plane = (cd >> (r >= 9 ? 4 : 0)) & 0xfu;
        want = lut16_value(p.lut, plane, lc, r % 9u);
    }
    else {
        want = p.want[r][(size_t)ys * p.want_stride + x];
    }
    p.counts[r].want = want;
    p.counts[r].got = p.got[r][(size_t)ys * p.got_stride + x];
}

uint32_t grid_for(const gcn10_gpu_ctx *ctx, const VerifyParams &p)
{
    const uint32_t trips = (p.n_groups + kThreads - 1u) / kThreads;
    const uint32_t tail = (p.W - p.groups_per_row * kPxPerLane) * p.rows;
    const uint32_t want = trips > (tail + kThreads - 1u) / kThreads ? trips : (tail + kThreads - 1u) / kThreads;
    const uint32_t cap = grid_cap(ctx, kGridPerCu);
    return want < cap ? (want ? want : 1u) : cap;
}

int fill_shape(VerifyParams &p, const char *who, int W, int rows, int y0, size_t got_stride)
{
    if (W <= 0 || rows < 0 || y0 < 0 || (uint64_t)W * (uint64_t)rows > 0x7fffffffull)
        return fail(GCN10_E_INVAL, "%s: W=%d rows=%d y0=%d (at most 2^31-1 pixels per call)", who, W, rows, y0);
    if (got_stride < (size_t)W)
        return fail(GCN10_E_INVAL, "%s: got_stride %zu < W=%d", who, got_stride, W);
    p.W = (uint32_t)W;
    p.rows = (uint32_t)rows;
    p.y0 = (uint32_t)y0;
    p.got_stride = got_stride;
    p.groups_per_row = p.W / kPxPerLane;
    p.n_groups = p.rows * p.groups_per_row;
    return GCN10_OK;
}

}  // namespace

extern "C" {

int gcn10_gpu_verify_strip(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                           unsigned cond_mask, unsigned table_mask, const uint8_t *const got[GCN10_N_RASTERS],
                           size_t got_stride, int y0, gcn10_verify_count *counts_dev, gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    const char *const who = "gcn10_gpu_verify_strip";
    hipStream_t s = as_stream(ctx, stream);
    VerifyParams p;
    memset(&p, 0, sizeof p);
    if ((rc = check_tables(ctx, who)) != GCN10_OK || (rc = bind_soil(ctx, who, W, s, cj, &p.soil)) != GCN10_OK ||
        (rc = check_masks(ctx, who, cond_mask, table_mask)) != GCN10_OK ||
        (rc = fill_shape(p, who, W, rows, y0, got_stride)) != GCN10_OK)
        return rc;
    if (rows == 0)
        return GCN10_OK;
    if (!esa || !cj || !got || !counts_dev)
        return fail(GCN10_E_INVAL, "gcn10_gpu_verify_strip: null pointer");
    for (int r = 0; r < GCN10_N_RASTERS; r++) {
        if (!selected(r, cond_mask, table_mask))
            continue;
        if (!got[r])
            return fail(GCN10_E_INVAL, "gcn10_gpu_verify_strip: got[%d] is null but selected", r);
        p.got[r] = got[r];
        p.sel |= 1u << r;
    }
    p.esa = esa;
    p.lut = ctx->d_lut16;
    p.counts = counts_dev;
    if (p.sel == (1u << GCN10_N_RASTERS) - 1u)
        hipLaunchKernelGGL(verify_strip_kernel<true>, dim3(grid_for(ctx, p)), dim3(kThreads), 0, s, p);
    else
        hipLaunchKernelGGL(verify_strip_kernel<false>, dim3(grid_for(ctx, p)), dim3(kThreads), 0, s, p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(verify_first_kernel<true>, dim3(1), dim3(64), 0, s, p);
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}

int gcn10_gpu_verify_buffers(gcn10_gpu_ctx *ctx, const uint8_t *const want[GCN10_N_RASTERS], size_t want_stride,
                             const uint8_t *const got[GCN10_N_RASTERS], size_t got_stride, int W, int rows, int y0,
                             unsigned raster_mask, gcn10_verify_count *counts_dev, gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (raster_mask == 0 || (raster_mask >> GCN10_N_RASTERS))
        return fail(GCN10_E_INVAL, "gcn10_gpu_verify_buffers: raster_mask 0x%x", raster_mask);
    VerifyParams p;
    memset(&p, 0, sizeof p);
    rc = fill_shape(p, "gcn10_gpu_verify_buffers", W, rows, y0, got_stride);
    if (rc)
        return rc;
    if (want_stride < (size_t)W)
        return fail(GCN10_E_INVAL, "gcn10_gpu_verify_buffers: want_stride %zu < W=%d", want_stride, W);
    if (rows == 0)
        return GCN10_OK;
    if (!want || !got || !counts_dev)
        return fail(GCN10_E_INVAL, "gcn10_gpu_verify_buffers: null pointer");
    for (int r = 0; r < GCN10_N_RASTERS; r++) {
        if (!(raster_mask & (1u << r)))
            continue;
        if (!want[r] || !got[r])
            return fail(GCN10_E_INVAL, "gcn10_gpu_verify_buffers: raster %d is selected but has a null pointer", r);
        p.want[r] = want[r];
        p.got[r] = got[r];
    }
    p.sel = raster_mask;
    p.want_stride = want_stride;
    p.counts = counts_dev;
    hipStream_t s = as_stream(ctx, stream);
    hipLaunchKernelGGL(verify_buffers_kernel, dim3(grid_for(ctx, p)), dim3(kThreads), 0, s, p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(verify_first_kernel<false>, dim3(1), dim3(64), 0, s, p);
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}

}  // extern "C"
