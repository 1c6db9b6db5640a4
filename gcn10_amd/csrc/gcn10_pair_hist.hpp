// gcn10_pair_hist.hpp -- the pieces the pair-histogram kernels share (gcn10_stats.hip: a whole strip;
// gcn10_zonal.hip, gcn10_zonal_rain.hip and gcn10_zonal_rains.hip: the spans of zones; gcn10_grid_rain.hip and gcn10_grid_rains.hip: the cells of a grid): the bin of a soil code, the key of a pixel, and the run folding of a
// lane's 16 pixels.  Why runs are folded: header comment of gcn10_stats.hip.
#ifndef GCN10_PAIR_HIST_HPP
#define GCN10_PAIR_HIST_HPP

#include <hip/hip_runtime.h>

#include <cstdint>

#include "gcn10_gpu_internal.hpp"

namespace gcn10 {
namespace pair_hist {

constexpr int kThreads = 256;
constexpr uint32_t kPxPerLane = 16;
constexpr int kBins = GCN10_PAIR_HIST_BINS;
constexpr int kHistWords = GCN10_PAIR_HIST_SIZE;       // [bin][landcover]

// soil code byte (drained plane | undrained plane << 4) -> dense bin: d == u -> d (0..5); a dual class
// (d = 4, u = 1..3) -> 5 + u (6..8).  Bins 9..15 stay empty.
__host__ __device__ inline uint32_t code_bin(uint32_t code)
{
    const uint32_t d = code & 15u, u = code >> 4;
    const uint32_t b = d == u ? d : 5u + u;
    return b < (uint32_t)kBins ? b : (uint32_t)kBins - 1u;
}

// the soil code of a bin (gcn10_gpu_pair_histogram_codes): the inverse of code_bin on the bins a code maps to
__host__ __device__ inline uint32_t bin_code(uint32_t bin)
{
    return bin < 6u ? bin * 0x11u : bin < 9u ? 4u | (bin - 5u) << 4 : 0x55u;
}

// key of pixel i of a lane: landcover in bits 0..7, soil code in bits 8..15
__device__ __forceinline__ uint32_t pair_key(const u32x4 &e, const u32x4 &s, uint32_t i)
{
    const uint32_t sel = 0x0c0c0400u + (i & 3u) * 0x00000101u;  // byte 0 <- e byte i&3, byte 1 <- s byte i&3
    return __builtin_amdgcn_perm(s[i >> 2], e[i >> 2], sel);
}

__device__ __forceinline__ void add_run(uint32_t *h, uint32_t key, uint32_t n)
{
    atomicAdd(&h[code_bin(key >> 8) * 256u + (key & 255u)], n);
}

__device__ __forceinline__ bool all_one_byte(const u32x4 &v)
{
    const uint32_t b = (v[0] & 255u) * 0x01010101u;
    return v[0] == b && v[1] == b && v[2] == b && v[3] == b;
}

// 16 pixels of a lane: runs of equal pairs folded in registers, one LDS add per run; a wave whose active lanes
// all hold one single pair adds once
__device__ __forceinline__ void count16(uint32_t *h, const u32x4 &e, const u32x4 &s)
{
    const uint32_t k0 = pair_key(e, s, 0);
    const bool one = all_one_byte(e) && all_one_byte(s);
    const uint32_t kw = __builtin_amdgcn_readfirstlane(k0);
    if (__all(one && k0 == kw)) {
        const uint64_t lanes = __ballot(1);
        if (__lane_id() == (uint32_t)__ffsll((long long)lanes) - 1u)
            add_run(h, kw, (uint32_t)__popcll(lanes) * kPxPerLane);
    }
    else if (one) {
        add_run(h, k0, kPxPerLane);
    }
    else {
        uint32_t cur = k0, n = 1u;
#pragma unroll
        for (uint32_t i = 1; i < kPxPerLane; i++) {
            const uint32_t k = pair_key(e, s, i);
            if (k != cur) {
                add_run(h, cur, n);
                cur = k;
                n = 0u;
            }
            n++;
        }
        add_run(h, cur, n);
    }
}

// pixels [a, b) of a lane's 16 (a span end of gcn10_zonal.hip, a cell edge of gcn10_grid_rain.hip): the run folding of
// count16 over the unmasked ones
__device__ __forceinline__ void count_masked(uint32_t *h, const u32x4 &e, const u32x4 &s, uint32_t a, uint32_t b)
{
    uint32_t cur = 0u, n = 0u;
#pragma unroll
    for (uint32_t i = 0; i < kPxPerLane; i++) {
        if (i >= a && i < b) {
            const uint32_t k = pair_key(e, s, i);
            if (n && k != cur) {
                add_run(h, cur, n);
                n = 0u;
            }
            cur = k;
            n++;
        }
    }
    if (n)
        add_run(h, cur, n);
}

// the row's last pixels (W not a multiple of 16): byte loads, nothing past the row end
__device__ __forceinline__ void count_tail(uint32_t *h, const uint8_t *erow, const uint8_t *srow, uint32_t m)
{
    uint32_t cur = (uint32_t)erow[0] | ((uint32_t)srow[0] << 8), n = 1u;
    for (uint32_t i = 1; i < m; i++) {
        const uint32_t k = (uint32_t)erow[i] | ((uint32_t)srow[i] << 8);
        if (k != cur) {
            add_run(h, cur, n);
            cur = k;
            n = 0u;
        }
        n++;
    }
    add_run(h, cur, n);
}

}  // namespace pair_hist
}  // namespace gcn10

#endif
