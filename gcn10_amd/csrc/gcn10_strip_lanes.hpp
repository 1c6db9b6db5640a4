// gcn10_strip_lanes.hpp -- which pixels a thread of a strip kernel that reads the soil tables works on.  Plain C++
// (no HIP header): the kernels and their host launch code call strip_lane_plan, and so does a host program of the
// tests.  Part of gcn10_gpu_internal.hpp.
#ifndef GCN10_STRIP_LANES_HPP
#define GCN10_STRIP_LANES_HPP

#include <cstdint>

#if defined(__HIPCC__)
#define GCN10_HOST_DEVICE __host__ __device__
#else
#define GCN10_HOST_DEVICE
#endif

namespace gcn10 {

// ---- lane plan of the strips that read the soil tables (W % 16 == 0) -------------------------------------------------
// A row is G = W/16 column groups of 16 pixels.  The strip is cut at row boundaries into `pieces` contiguous pieces:
// eight, one per XCD (workgroups with equal block & 7 share one), when XCD slabs are asked for, the grid is a multiple
// of 8 and a piece's T threads can hold a row; else one piece for the whole grid.  Thread t = local block * 256 + tid
// of a piece owns column group g = t % G and row phase rho = t / G for the whole launch; B = T / G rows are done per
// sub-trip, threads t >= B*G do nothing.  Sub-trip s = trip * ILP + u covers the piece's rows [s*B, s*B + B): the
// thread's 16-byte vector there is number s*B*G + t of the piece, so a sub-trip is one flat stream of consecutive
// vectors, and a thread's column group never changes.  B == 0: no plan (a row has more groups than the grid threads).
struct StripLanePlan {
    uint32_t G, B, T;
    uint32_t pieces;
    uint32_t row_lo, row_hi;    // the rows of this thread's piece
    uint32_t trips;             // loop trips of the piece, ILP sub-trips each
    uint32_t t, g, rho;
    bool active;                // t < B*G
};

constexpr uint32_t kStripThreads = 256;

// Rows per sub-trip for T threads: all that fit, or the next lower count that keeps the byte stride of a sub-trip
// (16*B*G) a multiple of 128 when that idles less than 5 % of the threads.
GCN10_HOST_DEVICE inline uint32_t strip_lane_rows(uint32_t T, uint32_t G)
{
    const uint32_t B = T / G;
    const uint32_t m = (G & 1u) ? 8u : (G & 2u) ? 4u : (G & 4u) ? 2u : 1u;     // B*G % 8 == 0 iff B % m == 0
    const uint32_t Ba = B - B % m;
    return Ba > 0u && (uint64_t)(T - Ba * G) * 20u < (uint64_t)T ? Ba : B;
}

GCN10_HOST_DEVICE inline StripLanePlan strip_lane_plan(uint32_t W, uint32_t rows, uint32_t grid, uint32_t block,
                                                         uint32_t tid, bool slabs, uint32_t ilp)
{
    StripLanePlan pl;
    pl.G = W / 16u;
    pl.pieces = 1u;
    pl.T = grid * kStripThreads;
    if (slabs && grid % 8u == 0u && (grid / 8u) * kStripThreads >= pl.G) {
        pl.pieces = 8u;
        pl.T = (grid / 8u) * kStripThreads;
    }
    pl.B = strip_lane_rows(pl.T, pl.G);
    const uint32_t piece = pl.pieces == 8u ? block & 7u : 0u;
    pl.row_lo = (uint32_t)((uint64_t)piece * rows / pl.pieces);
    pl.row_hi = (uint32_t)((uint64_t)(piece + 1u) * rows / pl.pieces);
    pl.t = (pl.pieces == 8u ? block >> 3 : block) * kStripThreads + tid;
    pl.g = pl.t % pl.G;
    pl.rho = pl.t / pl.G;
    pl.active = pl.rho < pl.B;
    const uint32_t per_trip = pl.B * ilp;
    pl.trips = per_trip ? (pl.row_hi - pl.row_lo + per_trip - 1u) / per_trip : 0u;
    return pl;
}

}  // namespace gcn10

#endif
