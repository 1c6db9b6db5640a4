// gcn10_deflate_fused_internal.hpp -- what passes F-A (gcn10_deflate_fused_stats.hpp) and F-C
// (gcn10_deflate_fused_emit.hpp) of the fused tile encoder both need: the job they are launched with, the group
// size, the token stream F-A hands to F-C, and the class ids of four pixels.  One translation unit,
// gcn10_deflate_fused.hip, includes all three: FusedJob names the kernels' argument and so is part of their symbols,
// which stay those of the unnamed namespace they have always had (profiles of earlier runs stay comparable).
#ifndef GCN10_DEFLATE_FUSED_INTERNAL_HPP
#define GCN10_DEFLATE_FUSED_INTERNAL_HPP

#include <hip/hip_runtime.h>

#include <cstdint>

#include "gcn10_deflate_internal.hpp"
#include "gcn10_gpu.h"
#include "gcn10_gpu_internal.hpp"
#include "gcn10_soil_readers.hpp"

using namespace gcn10_deflate;

namespace {

constexpr int kGroup = 6;            // rasters emitted by one workgroup of pass F-C

struct FusedJob {
    const uint8_t *esa;
    gcn10::SoilView soil;
    const uint8_t *class_of;        // [36][256]; class_val [18][256] follows
    uint16_t *tok;                  // [positions][kTokStride] token stream of each tile position (F-A -> F-C)
    uint32_t *n_tok;                // [positions] its length, end-of-block token included
    uint32_t seg_align;             // every raster's extent of the strip starts at a multiple of this (option arena_segment_align)
    uint32_t n_sel;                 // selected rasters, ascending
    uint8_t sel[GCN10_N_RASTERS];
    TileJob t;
};

__device__ __forceinline__ uint32_t compact_code(uint32_t code)
{
    return (code & 15u) * 6u + (code >> 4);
}

// Class ids of pixels (x..x+3, y) of the strip, one per byte; class 0 outside the raster.
__device__ __forceinline__ uint32_t class_pixels4(const FusedJob &job, uint32_t x, uint32_t y,
                                                  const uint8_t *class_of_lds)
{
    typedef uint32_t u32_u __attribute__((aligned(1)));
    const uint32_t W = job.t.W;
    uint32_t out = 0;
    if (y < job.t.rows && x < W) {
        const uint8_t *pe = job.esa + (size_t)y * W + x;
        // hx rows are padded by >= 16 bytes past W: a 4-byte read starting below W is safe
        const uint32_t c4 = *reinterpret_cast<const u32_u *>(job.soil.ptr(y, x));
        uint32_t e4 = 0;
        if (x + 4u <= W) {
            e4 = *reinterpret_cast<const u32_u *>(pe);
        }
        else {
            for (uint32_t k = 0; x + k < W; k++)
                e4 |= (uint32_t)pe[k] << (8 * k);
        }
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
            if (x + q < W) {
                const uint32_t lc = (e4 >> (8 * q)) & 0xffu;
                const uint32_t cc = compact_code((c4 >> (8 * q)) & 0xffu);
                out |= (uint32_t)class_of_lds[cc * 256u + lc] << (8 * q);
            }
        }
    }
    return out;
}

// The token stream pass F-C reads, 16 bits per token, rows back to back:
//   0x0000 | class                                  literal
//   0x8000 | length code | extra value << 5 | far << 10   match (far: distance 256, else 1)
//   0x4000                                          end of block
constexpr uint32_t kTokMatch = 0x8000u, kTokEnd = 0x4000u;
constexpr uint32_t kTokStride = kTileBytes + 64;    // tokens per tile position, worst case + the end token

}  // namespace

#endif
