// gcn10_device_util.hpp -- what the kernels of the strips, the prepared soil tile and the reference's per-function
// entry points share: the launch constants, the soil code byte, 16-byte lane accesses and the workgroup -> chunk
// mapping.  Written for gfx950 only: 64-lane waves, 16-byte per-lane global accesses (1 KiB per wave instruction).
#ifndef GCN10_DEVICE_UTIL_HPP
#define GCN10_DEVICE_UTIL_HPP

#include "gcn10_soil_readers.hpp"

namespace gcn10 {

// ------------------------------------------------------------------------
// constants shared by host and device
// ------------------------------------------------------------------------
constexpr int kThreads = 256;           // 4 waves per workgroup
constexpr int kPxPerLane = 16;          // one dwordx4 per lane per stream
constexpr int kChunk = kThreads * kPxPerLane;   // 4096 px per workgroup step
constexpr int kInvalidPlane = kPlanes - 1;  // soil groups 0..4 + the "invalid" plane

// soil code byte: low nibble = plane for "drained", high nibble = "undrained".
// src/cn.c:92-110 followed by the `soil_group < 5` test of src/cn.c:123-124.
__host__ __device__ inline uint8_t soil_code(uint8_t h)
{
    uint8_t d, u;
    if (h >= 11 && h <= 14) {
        d = 4;                  // drained: every dual class acts as D
        u = (uint8_t)(h - 10);  // undrained: 11..14 -> 1..4
    }
    else {
        d = u = (h < 5) ? h : (uint8_t)kInvalidPlane;
    }
    return (uint8_t)(d | (u << 4));
}

// ------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------

__device__ __forceinline__ u32x4 load16_aligned_nt(const uint8_t *p)
{
    return __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
}

__device__ __forceinline__ u32x4 load16_aligned(const uint8_t *p)
{
    return *reinterpret_cast<const u32x4 *>(p);
}

__device__ __forceinline__ u32x4 load16_any(const uint8_t *p)
{
    // gfx950 runs with unaligned global access enabled; tell the compiler the
    // pointer is only byte aligned and let it pick the widest legal load.
    typedef u32x4 u32x4_u __attribute__((aligned(1)));
    return *reinterpret_cast<const u32x4_u *>(p);
}

template <bool NT = true>
__device__ __forceinline__ void store16(uint8_t *p, u32x4 v)
{
    if (NT)
        __builtin_nontemporal_store(v, reinterpret_cast<u32x4 *>(p));
    else
        *reinterpret_cast<u32x4 *>(p) = v;
}

// cj[i] for a wave-uniform i through the scalar data cache (s_load_dword):
// constant-address-space loads with a uniform address select SMEM, which has
// its own counter (lgkmcnt) and does not queue behind vector memory traffic.
// cj is written by a copy that completed before this kernel started.
__device__ __forceinline__ int32_t scalar_load_i32(const int32_t *base, uint32_t i)
{
    typedef const int32_t __attribute__((address_space(4))) *const_ptr_t;
    const_ptr_t cp = (const_ptr_t)(uintptr_t)base;
    return cp[__builtin_amdgcn_readfirstlane(i)];
}

// Workgroup -> chunk mapping.  Workgroups are dealt round-robin over the 8
// XCDs (b and b+8 share one L2), so give each XCD a contiguous slab of the
// strip: the x-expanded soil rows a slab re-reads then stay in that XCD's L2.
__device__ __forceinline__ uint32_t first_chunk(uint32_t nchunks, uint32_t &step,
                                                uint32_t &end, bool xcd_slabs)
{
    uint32_t nb = gridDim.x;
    uint32_t b = blockIdx.x;
    if (xcd_slabs && nb % 8u == 0u && nchunks >= nb) {
        uint32_t xcd = b & 7u;
        uint32_t per = (nchunks + 7u) / 8u;
        uint32_t lo = xcd * per;
        uint32_t hi = lo + per < nchunks ? lo + per : nchunks;
        step = nb / 8u;
        end = hi;
        return lo + (b >> 3);
    }
    step = nb;
    end = nchunks;
    return b;
}

inline bool aligned16(const void *p)
{
    return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

inline int popcount(unsigned v)
{
    return __builtin_popcount(v);
}

}  // namespace gcn10

#endif
