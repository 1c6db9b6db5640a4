// gcn10_grid_rain_piece.hpp -- what the two kernels that sum a model grid from pair histograms share
// (gcn10_grid_rain.hip: one table per cell; gcn10_grid_rains.hip: k tables per cell): the item, the walk of the pieces
// of cells in it, the counting of a piece and the pack of its non-zero bins.  What a kernel does with the packed bins is
// its own.  P is the kernel's parameter block: esa, soil, W, rows, cellx, celly, ncx, ncy, chunks and band_rows as
// RainParams of gcn10_grid_rain.hip names them.
#ifndef GCN10_GRID_RAIN_PIECE_HPP
#define GCN10_GRID_RAIN_PIECE_HPP

#include <hip/hip_runtime.h>

#include <cstdint>

#include "gcn10_grid_internal.hpp"
#include "gcn10_pair_hist.hpp"

namespace gcn10 {
namespace rain_piece {

using namespace gcn10::pair_hist;

constexpr uint32_t kWave = 64;
constexpr uint32_t kItemCols = GCN10_GPU_RAIN_ITEM_COLS, kItemRows = GCN10_GPU_RAIN_ITEM_ROWS;
constexpr uint32_t kMinBandRows = 16;
constexpr uint32_t kChunkWords = 4u * kWave;                // histogram words a wave reads at a time
static_assert(kItemCols % kPxPerLane == 0 && kItemCols * kItemRows <= 65535u, "an item's counts fit 16 bits");
static_assert(kHistWords % kChunkWords == 0, "the pack reads whole chunks");

// The run of equal entries of `map` that begins at i < end: its value, and where it ends (<= end).  Called by the whole
// wave with the same arguments.
__device__ __forceinline__ uint32_t run_end(const int32_t *map, uint32_t i, uint32_t end, int32_t &value)
{
    value = __builtin_amdgcn_readfirstlane(map[i]);
    for (uint32_t j = i;; j += kWave) {
        const uint32_t k = j + __lane_id();
        const uint64_t differs = __ballot(k >= end || map[k] != value);
        if (differs)
            return j + (uint32_t)__ffsll((long long)differs) - 1u;
    }
}

// a unit of a piece: the 16-column group at gx of strip row y, of which the piece has columns [a, b)
struct Unit {
    u32x4 e, s;
    uint32_t y, gx, a, b;
};

template <typename P>
__device__ __forceinline__ void fetch(const P &p, uint32_t u, uint32_t ng, uint32_t g0, uint32_t xa, uint32_t xb,
                                      uint32_t ya, Unit &t)
{
    const uint32_t r = u / ng;
    t.y = ya + r;
    t.gx = (g0 + (u - r * ng)) * kPxPerLane;
    t.a = max(t.gx, xa);
    t.b = min(t.gx + kPxPerLane, xb);
    if (t.gx + kPxPerLane <= p.W) {
        t.e = *reinterpret_cast<const u32x4_u *>(p.esa + (size_t)t.y * p.W + t.gx);
        t.s = *reinterpret_cast<const u32x4 *>(p.soil.ptr(t.y, t.gx));
    }
}

template <typename P>
__device__ __forceinline__ void count(const P &p, uint32_t *h, const Unit &t)
{
    if (t.gx + kPxPerLane <= p.W) {
        if (t.b - t.a == kPxPerLane)
            count16(h, t.e, t.s);
        else
            count_masked(h, t.e, t.s, t.a - t.gx, t.b - t.gx);
    }
    else {
        // the row's last group, W no multiple of 16: bytes, nothing past the row end
        count_tail(h, p.esa + (size_t)t.y * p.W + t.a, p.soil.ptr(t.y, t.a), t.b - t.a);
    }
}

// Columns [xa, xb) x rows [ya, yb), all inside the wave's item, counted into h, which is all zero before; then the
// non-zero bins packed to h[0 .. m) as bin << 16 | count, every other word of h zero.  Returns m, the same for the whole
// wave.
template <typename P>
__device__ __forceinline__ uint32_t count_and_pack(const P &p, uint32_t *h, uint32_t xa, uint32_t xb, uint32_t ya,
                                                   uint32_t yb)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t g0 = xa / kPxPerLane, ng = (xb - 1u) / kPxPerLane - g0 + 1u, units = (yb - ya) * ng;

    // the next unit's loads in flight over this unit's LDS adds
    Unit cur = {}, next = {};
    if (lane < units)
        fetch(p, lane, ng, g0, xa, xb, ya, cur);
    for (uint32_t u = lane; u < units; u += kWave) {
        if (u + kWave < units)
            fetch(p, u + kWave, ng, g0, xa, xb, ya, next);
        count(p, h, cur);
        cur = next;
    }
    __syncthreads();

    // before a chunk is read, m is at most the words read so far, and a chunk is cleared before bins are packed into it
    uint32_t m = 0u;
    for (uint32_t j = 0; j < (uint32_t)kHistWords; j += kChunkWords) {
        u32x4 *const at = reinterpret_cast<u32x4 *>(h + j + 4u * lane);
        const u32x4 v = *at;
        if (!__any((v[0] | v[1] | v[2] | v[3]) != 0u))
            continue;
        *at = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const bool nz = v[k] != 0u;
            const uint64_t who = __ballot(nz);
            if (nz)
                h[m + (uint32_t)__popcll(who & ((1ull << lane) - 1ull))] = (j + 4u * lane + k) << 16 | v[k];
            m += (uint32_t)__popcll(who);
        }
    }
    __syncthreads();
    return m;
}

// The body of a sums kernel: the histogram cleared, then every piece of a cell in the workgroup's item handed to
// piece(xa, xb, ya, yb, cx, cy), wave uniform throughout.  A run of the maps that is no cell is stepped over.
template <typename P, typename F>
__device__ __forceinline__ void walk_item(const P &p, uint32_t *h, F piece)
{
    for (uint32_t i = 4u * threadIdx.x; i < (uint32_t)kHistWords; i += kChunkWords)
        *reinterpret_cast<u32x4 *>(h + i) = u32x4{0u, 0u, 0u, 0u};
    __syncthreads();

    const uint32_t band = blockIdx.x / p.chunks, chunk = blockIdx.x - band * p.chunks;
    const uint32_t x0 = chunk * kItemCols, x1 = min(x0 + kItemCols, p.W);
    const uint32_t y0 = band * p.band_rows, y1 = min(y0 + p.band_rows, p.rows);
    for (uint32_t ya = y0; ya < y1;) {
        int32_t cy;
        const uint32_t yb = run_end(p.celly, ya, y1, cy);
        if ((uint32_t)cy < p.ncy) {             // a negative entry is >= ncy
            for (uint32_t xa = x0; xa < x1;) {
                int32_t cx;
                const uint32_t xb = run_end(p.cellx, xa, x1, cx);
                if ((uint32_t)cx < p.ncx)
                    piece(xa, xb, ya, yb, (uint32_t)cx, (uint32_t)cy);
                xa = xb;
            }
        }
        ya = yb;
    }
}

}  // namespace rain_piece
}  // namespace gcn10

#endif
