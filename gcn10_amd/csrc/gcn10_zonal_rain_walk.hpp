// gcn10_zonal_rain_walk.hpp -- what the two zonal rain kernels share (gcn10_zonal_rain.hip: one table per item;
// gcn10_zonal_rains.hip: a tuple of up to eight): the LDS of a workgroup's walk, the counting of an item's spans into the
// pair histogram at hand, and the listing of the non-zero bins at a flush.  What a flush then does with the list differs.
#ifndef GCN10_ZONAL_RAIN_WALK_HPP
#define GCN10_ZONAL_RAIN_WALK_HPP

#include <hip/hip_runtime.h>

#include <cstdint>

#include "gcn10_grid_internal.hpp"
#include "gcn10_pair_hist.hpp"

namespace gcn10 {
namespace zonal_rain_walk {

using namespace gcn10::pair_hist;

// as gcn10_zonal.hip has it (the same workgroup, with the list of a flush 29 KiB of LDS)
constexpr int kGridPerCu = 4;
constexpr uint32_t kWaves = kThreads / 64;

// the spans at hand (256 of an item) and the prefix sums of their group counts
struct WalkLds {
    uint32_t pre[kThreads + 1];         // groups before span j of the spans at hand
    int32_t sy[kThreads], sx0[kThreads], sx1[kThreads];
    uint32_t wave_sum[kWaves];
};

// The pixels of spans [first_span, first_span + n_spans) into h: 16-pixel groups dealt to the lanes.  Workgroup uniform;
// ends with a barrier, after which lds may be written again (h holds the counts of every lane only after another one).
__device__ __forceinline__ void count_item(const uint8_t *esa, const SoilView &soil, uint32_t W,
                                           const gcn10_zone_span *spans, uint32_t first_span, uint32_t n_spans,
                                           uint32_t *h, WalkLds &lds)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t s0 = 0; s0 < n_spans; s0 += kThreads) {
        const uint32_t ns = min((uint32_t)kThreads, n_spans - s0);
        uint32_t g = 0u;
        if (tid < ns) {
            const gcn10_zone_span sp = spans[first_span + s0 + tid];
            lds.sy[tid] = sp.y;
            lds.sx0[tid] = sp.x0;
            lds.sx1[tid] = sp.x1;
            g = (((uint32_t)sp.x1 - 1u) >> 4) - ((uint32_t)sp.x0 >> 4) + 1u;
        }
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t t = __shfl_up(g, d, 64);
            if (lane >= d)
                g += t;
        }
        if (lane == 63u)
            lds.wave_sum[wave] = g;
        __syncthreads();
        for (uint32_t w = 0; w < wave; w++)
            g += lds.wave_sum[w];
        lds.pre[tid + 1] = g;
        if (tid == 0)
            lds.pre[0] = 0u;
        __syncthreads();
        const uint32_t total = lds.pre[ns];

        for (uint32_t q = tid; q < total; q += kThreads) {
            // the span of group q: the last j with pre[j] <= q
            uint32_t lo = 0u, hi = ns;
            while (hi - lo > 1u) {
                const uint32_t mid = (lo + hi) >> 1;
                if (lds.pre[mid] <= q)
                    lo = mid;
                else
                    hi = mid;
            }
            const uint32_t x0 = (uint32_t)lds.sx0[lo], x1 = (uint32_t)lds.sx1[lo], y = (uint32_t)lds.sy[lo];
            const uint32_t gx = ((x0 >> 4) + (q - lds.pre[lo])) << 4;       // first column of the group
            const uint32_t a = max(gx, x0), b = min(gx + kPxPerLane, x1);
            const uint8_t *erow = esa + (size_t)y * W + gx;
            const uint8_t *srow = soil.ptr(y, gx);
            if (gx + kPxPerLane <= W) {
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

// The non-zero bins of h -- a few dozen of the 4096 -- into list, their number into *n_list, which the caller cleared
// behind a barrier; the caller's barrier follows.  They are listed first and then dealt one (bin, condition) to a
// thread: the bins of one landcover class lie 256 words apart, so a strided scan that reduced on the spot would leave all
// of a class's bins, each with its chain of dependent loads (image row, then weights), to ONE thread.
__device__ __forceinline__ void list_bins(const uint32_t *h, uint16_t *list, uint32_t *n_list)
{
    for (uint32_t j = 4u * threadIdx.x; j < (uint32_t)kHistWords; j += 4u * kThreads) {
        const u32x4 v = *reinterpret_cast<const u32x4 *>(h + j);
#pragma unroll
        for (uint32_t k = 0; k < 4; k++)
            if (v[k])
                list[atomicAdd(n_list, 1u)] = (uint16_t)(j + k);
    }
}

// the nine values of the (bin, condition) at hand: the image row of the bin's soil code under that condition
__device__ __forceinline__ void bin_values(const uint8_t *lut, uint32_t bin, uint32_t cond, uint32_t v[9])
{
    const uint32_t lc = bin & 255u, code = bin_code(bin >> 8);
    const u32x4 r = *reinterpret_cast<const u32x4 *>(lut16_row(lut, (code >> (4u * cond)) & 15u, lc));
#pragma unroll
    for (uint32_t t = 0; t < 9; t++)
        v[t] = (r[t >> 2] >> (8u * (t & 3u))) & 255u;
}

}  // namespace zonal_rain_walk
}  // namespace gcn10

#endif
