// gcn10_zonal.hip -- the (landcover, soil code) pair histogram of gcn10_stats.hip restricted to the pixels of zones
// (config key zonal=1, DESIGN.md "Zonal composites").
//
// The host hands over spans {y, x0, x1, zone} sorted by zone and work items, runs of consecutive spans of one zone
// with a bounded number of pixels (gcn10_zones_build_plan).  A workgroup takes a CONTIGUOUS run of items, not a grid
// stride: items are sorted by zone, so it sees few zones and keeps the 16 KiB LDS histogram of pair_histogram_kernel
// for the zone at hand; nonzero bins go to hist[zone] with 64-bit global atomics when the zone changes and at the end.
//
// Within an item the unit of work is a 16-pixel column group of a span -- the groups of the soil row, so the soil
// load is aligned as in pair_histogram_kernel and only the landcover load is not.  Up to 256 spans at a time are
// laid into LDS with the prefix sum of their group counts, and the groups are dealt to the lanes: lane l takes
// groups l, l + 256, ... and finds each one's span with a binary search of the prefix sums.  A group that the span
// covers whole is counted by count16; one the span begins or ends in masks the pixels before x0 and from x1 on with
// the same run folding; the last group of a row whose width is no multiple of 16 is read byte by byte (count_tail),
// so nothing is read beyond esa + W * rows or a soil row's stride.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gcn10_gpu_internal.hpp"
#include "gcn10_pair_hist.hpp"
#include "gcn10_soil_readers.hpp"

using namespace gcn10;
using namespace gcn10::pair_hist;

namespace {

// Workgroups per CU at most: the value measured for pair_histogram_kernel (20 KiB of LDS each here), taken over and
// not swept on its own.  The span and item bounds of the host builder were swept against it (tools/bench_zonal.py
// --bounds, profiles/zonal/kernel_bounds.json): what matters is that the items outnumber these workgroups.
constexpr int kZonalGridPerCu = 4;
constexpr uint32_t kWaves = kThreads / 64;

struct ZonalParams {
    const uint8_t *esa;             // strip, W x rows, row major
    SoilView soil;                  // x-expanded soil codes, soil row of every strip row
    const gcn10_zone_span *spans;
    const gcn10_zone_item *items;
    unsigned long long *hist;       // [n_zones][kHistWords]
    uint32_t W, n_items, items_per_wg;
};

// the workgroup's histogram to the zone's, nonzero bins only, and cleared for the next zone
__device__ __forceinline__ void flush_zone(uint32_t *h, unsigned long long *dst)
{
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < (uint32_t)kHistWords; i += kThreads) {
        const uint32_t v = h[i];
        if (v) {
            atomicAdd(&dst[i], (unsigned long long)v);
            h[i] = 0u;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(kThreads) void zonal_pair_histogram_kernel(const ZonalParams p)
{
    __shared__ uint32_t h[kHistWords];
    __shared__ uint32_t pre[kThreads + 1];          // groups before span j of the spans at hand
    __shared__ int32_t sy[kThreads], sx0[kThreads], sx1[kThreads];
    __shared__ uint32_t wave_sum[kWaves];

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t i = tid; i < (uint32_t)kHistWords; i += kThreads)
        h[i] = 0u;
    __syncthreads();

    const uint32_t first = blockIdx.x * p.items_per_wg;
    const uint32_t last = min(first + p.items_per_wg, p.n_items);
    int32_t cur_zone = -1;
    for (uint32_t it = first; it < last; it++) {            // workgroup uniform throughout
        const uint32_t first_span = p.items[it].first_span, n_spans = p.items[it].n_spans;
        const int32_t zone = p.spans[first_span].zone;
        if (zone != cur_zone) {
            if (cur_zone >= 0)
                flush_zone(h, p.hist + (size_t)cur_zone * kHistWords);
            cur_zone = zone;
        }
        for (uint32_t s0 = 0; s0 < n_spans; s0 += kThreads) {
            const uint32_t ns = min((uint32_t)kThreads, n_spans - s0);
            // the spans at hand and the prefix sums of their group counts
            uint32_t g = 0u;
            if (tid < ns) {
                const gcn10_zone_span sp = p.spans[first_span + s0 + tid];
                sy[tid] = sp.y;
                sx0[tid] = sp.x0;
                sx1[tid] = sp.x1;
                g = (((uint32_t)sp.x1 - 1u) >> 4) - ((uint32_t)sp.x0 >> 4) + 1u;
            }
#pragma unroll
            for (uint32_t d = 1; d < 64u; d <<= 1) {
                const uint32_t t = __shfl_up(g, d, 64);
                if (lane >= d)
                    g += t;
            }
            if (lane == 63u)
                wave_sum[wave] = g;
            __syncthreads();
            for (uint32_t w = 0; w < wave; w++)
                g += wave_sum[w];
            pre[tid + 1] = g;
            if (tid == 0)
                pre[0] = 0u;
            __syncthreads();
            const uint32_t total = pre[ns];

            for (uint32_t q = tid; q < total; q += kThreads) {
                // the span of group q: the last j with pre[j] <= q
                uint32_t lo = 0u, hi = ns;
                while (hi - lo > 1u) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (pre[mid] <= q)
                        lo = mid;
                    else
                        hi = mid;
                }
                const uint32_t x0 = (uint32_t)sx0[lo], x1 = (uint32_t)sx1[lo], y = (uint32_t)sy[lo];
                const uint32_t gx = ((x0 >> 4) + (q - pre[lo])) << 4;       // first column of the group
                const uint32_t a = max(gx, x0), b = min(gx + kPxPerLane, x1);
                const uint8_t *erow = p.esa + (size_t)y * p.W + gx;
                const uint8_t *srow = p.soil.ptr(y, gx);
                if (gx + kPxPerLane <= p.W) {
                    typedef u32x4 u32x4_u __attribute__((aligned(1)));
                    const u32x4 e = *reinterpret_cast<const u32x4_u *>(erow);
                    const u32x4 s = *reinterpret_cast<const u32x4 *>(srow);
                    if (b - a == kPxPerLane)
                        count16(h, e, s);
                    else
                        count_masked(h, e, s, a - gx, b - gx);
                }
                else {
                    // the row's last group, W no multiple of 16: bytes, nothing past the row end
                    count_tail(h, erow + (a - gx), srow + (a - gx), b - a);
                }
            }
            __syncthreads();        // sy / sx0 / sx1 / pre are rewritten by the next 256 spans
        }
    }
    if (cur_zone >= 0)
        flush_zone(h, p.hist + (size_t)cur_zone * kHistWords);
}

}  // namespace

extern "C" {

int gcn10_gpu_zonal_pair_histogram(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                                   const gcn10_zone_span *spans_dev, const gcn10_zone_item *items_dev, size_t n_items,
                                   int n_zones, unsigned long long *hist_dev, gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (n_items == 0)
        return GCN10_OK;
    ZonalParams p = {};
    if ((rc = bind_soil(ctx, "gcn10_gpu_zonal_pair_histogram", W, as_stream(ctx, stream), cj, &p.soil)) != GCN10_OK)
        return rc;
    if (!esa || !cj || !spans_dev || !items_dev || !hist_dev || W <= 0 || rows <= 0 || n_zones <= 0 ||
        n_items > 0xffffffffu)
        return fail(GCN10_E_INVAL, "gcn10_gpu_zonal_pair_histogram: bad arguments W=%d rows=%d zones=%d items=%zu", W,
                    rows, n_zones, n_items);
    p.esa = esa;
    p.spans = spans_dev;
    p.items = items_dev;
    p.hist = hist_dev;
    p.W = (uint32_t)W;
    p.n_items = (uint32_t)n_items;
    const uint64_t cap = grid_cap(ctx, kZonalGridPerCu);
    const uint32_t grid = (uint32_t)(n_items < cap ? n_items : cap);
    p.items_per_wg = (p.n_items + grid - 1u) / grid;
    hipLaunchKernelGGL(zonal_pair_histogram_kernel, dim3(grid), dim3(kThreads), 0, as_stream(ctx, stream), p);
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}

}  // extern "C"
