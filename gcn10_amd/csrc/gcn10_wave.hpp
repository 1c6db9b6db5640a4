// gcn10_wave.hpp -- what the kernels of the codecs (the tile encoders, gcn10_inflate.hip) do across the 64 lanes of a
// wave: a wave-uniform value in a scalar register, a wave-level barrier, prefix sum and total with DPP adds.
#ifndef GCN10_WAVE_HPP
#define GCN10_WAVE_HPP

#include <hip/hip_runtime.h>

#include <cstdint>

namespace gcn10 {

__device__ __forceinline__ uint32_t uniform(uint32_t v)
{
    return __builtin_amdgcn_readfirstlane(v);
}

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Inclusive prefix sum over the 64 lanes with DPP adds (no LDS traffic): three shifted adds of
// the input give sums over 4 lanes, row_shr:4 / row_shr:8 complete the rows of 16, row_bcast:15
// and row_bcast:31 carry the row totals on.
__device__ __forceinline__ uint32_t wave_scan(uint32_t x)
{
    uint32_t r = x;
    r += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);     // row_shr:1
    r += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);     // row_shr:2
    r += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x113, 0xf, 0xf, false);     // row_shr:3
    r += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)r, 0x114, 0xf, 0xe, false);     // row_shr:4, lanes 4..15
    r += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)r, 0x118, 0xf, 0xc, false);     // row_shr:8, lanes 8..15
    r += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)r, 0x142, 0xa, 0xf, false);     // row_bcast:15 -> rows 1, 3
    r += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)r, 0x143, 0xc, 0xf, false);     // row_bcast:31 -> rows 2, 3
    return r;
}

// Sum over the 64 lanes with DPP adds (no LDS round trips), in every lane of the last row (48..63): quads, rows of 16,
// then row_bcast:15 / row_bcast:31 carry the row totals on.  What the other lanes hold is a partial sum.
__device__ __forceinline__ uint32_t wave_total_in_last_row(uint32_t x)
{
    uint32_t r = x;
    r += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)r, 0xb1, 0xf, 0xf, false);      // quad_perm [1,0,3,2]
    r += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)r, 0x4e, 0xf, 0xf, false);      // quad_perm [2,3,0,1]
    r += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)r, 0x141, 0xf, 0xf, false);     // row_half_mirror
    r += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)r, 0x140, 0xf, 0xf, false);     // row_mirror
    r += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)r, 0x142, 0xa, 0xf, false);     // row_bcast:15 -> rows 1, 3
    r += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)r, 0x143, 0xc, 0xf, false);     // row_bcast:31 -> rows 2, 3
    return r;
}

// Sum over the 64 lanes, wave-uniform
__device__ __forceinline__ uint32_t wave_total(uint32_t x)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_total_in_last_row(x), 63);
}

}  // namespace gcn10

#endif
