// Host check of gcn10::strip_lane_plan (gcn10_amd/csrc/gcn10_strip_lanes.hpp), the lane-to-pixel mapping of the strip
// kernels that read the soil tables.  Arguments: groups of W rows grid slabs ilp.  For every group, every thread of
// the grid is walked through its trips with the arithmetic the kernel uses (issue_lane_trip of gcn10_strip.hip):
//   * every 16-byte vector of the strip is visited exactly once,
//   * a thread never leaves its column group,
//   * the pieces begin at row boundaries and tile the strip,
//   * inside a wave the lanes behind the row end are one row further than the first lane, no other row occurs.
// Prints one line per group: "W rows grid slabs ilp pieces B trips".  B == 0: no plan, nothing walked.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gcn10_strip_lanes.hpp"

#define CHECK(cond, ...)                   \
    do {                                   \
        if (!(cond)) {                     \
            fprintf(stderr, __VA_ARGS__);  \
            fprintf(stderr, "\n");         \
            return 1;                      \
        }                                  \
    } while (0)

static int walk(uint32_t W, uint32_t rows, uint32_t grid, bool slabs, uint32_t ilp)
{
    const gcn10::StripLanePlan p0 = gcn10::strip_lane_plan(W, rows, grid, 0, 0, slabs, ilp);
    uint32_t max_trips = 0;
    if (p0.B == 0) {
        CHECK((uint64_t)grid * 256u < W / 16u, "B == 0 although the grid has a thread for every group");
        printf("%u %u %u %d %u %u 0 0\n", W, rows, grid, (int)slabs, ilp, p0.pieces);
        return 0;
    }
    const uint32_t G = W / 16u;
    std::vector<uint8_t> seen((size_t)rows * G, 0);
    std::vector<uint8_t> row_piece(rows, 0xff);
    for (uint32_t block = 0; block < grid; block++) {
        for (uint32_t wave = 0; wave < 4; wave++) {
            uint32_t g_first = 0, rho_first = 0;
            for (uint32_t lane = 0; lane < 64; lane++) {
                const uint32_t tid = wave * 64 + lane;
                const gcn10::StripLanePlan pl = gcn10::strip_lane_plan(W, rows, grid, block, tid, slabs, ilp);
                CHECK(pl.G == G && pl.B == p0.B && pl.T == p0.T && pl.pieces == p0.pieces, "plan differs between threads");
                CHECK(pl.g < G && pl.t == pl.rho * G + pl.g, "block %u tid %u: t != rho*G + g", block, tid);
                CHECK(pl.active == (pl.t < pl.B * G), "block %u tid %u: active", block, tid);
                CHECK(pl.row_lo <= pl.row_hi && pl.row_hi <= rows, "block %u: piece rows", block);
                const uint32_t piece = pl.pieces == 8 ? block & 7u : 0u;
                const gcn10::StripLanePlan pb = gcn10::strip_lane_plan(W, rows, grid, piece, 0, slabs, ilp);
                CHECK(pl.row_lo == pb.row_lo && pl.row_hi == pb.row_hi && pl.trips == pb.trips,
                      "block %u tid %u: the piece differs between its threads", block, tid);
                for (uint32_t y = pl.row_lo; tid == 0 && y < pl.row_hi; y++) {
                    CHECK(row_piece[y] == 0xff || row_piece[y] == piece, "row %u in two pieces", y);
                    row_piece[y] = (uint8_t)piece;
                }
                if (lane == 0) {
                    g_first = pl.g;
                    rho_first = pl.rho;
                }
                // the kernel's wave-uniform row: the first lane's, one further behind the row end
                const bool wrap = pl.g < g_first;
                CHECK(pl.rho == rho_first + (wrap ? 1u : 0u), "block %u tid %u: a wave spans more than one row end", block,
                      tid);
                if (pl.trips > max_trips)
                    max_trips = pl.trips;
                // the kernel's per-lane values (lane_prologue)
                const uint64_t base = ((uint64_t)pl.row_lo * G + pl.t) * 16u;
                const uint64_t lim = pl.active ? (uint64_t)pl.row_hi * W : 0u;
                const uint64_t sub_px = (uint64_t)pl.B * W;
                for (uint32_t trip = 0; trip < pl.trips; trip++) {
                    for (uint32_t u = 0; u < ilp; u++) {
                        const uint64_t s = (uint64_t)trip * ilp + u;
                        const uint64_t i0 = base + s * sub_px;
                        CHECK(i0 <= 0xffffffffull, "pixel index leaves 32 bits");
                        if (i0 >= lim)
                            continue;
                        const uint64_t v = i0 / 16u;
                        CHECK(v < (uint64_t)rows * G, "vector %llu outside the strip", (unsigned long long)v);
                        CHECK(v % G == pl.g, "block %u tid %u leaves column group %u", block, tid, pl.g);
                        CHECK(v == (uint64_t)pl.row_lo * G + s * pl.B * G + pl.t, "vector number");
                        const uint64_t y = v / G;
                        CHECK(y == pl.row_lo + s * pl.B + pl.rho && y >= pl.row_lo && y < pl.row_hi,
                              "block %u tid %u: row %llu outside its piece", block, tid, (unsigned long long)y);
                        CHECK(seen[v] == 0, "vector %llu visited twice", (unsigned long long)v);
                        seen[v] = 1;
                    }
                }
                // nothing is left behind the last trip
                CHECK(!pl.active || base + (uint64_t)pl.trips * ilp * sub_px >= lim, "block %u tid %u: trips end early",
                      block, tid);
            }
        }
    }
    for (size_t v = 0; v < seen.size(); v++)
        CHECK(seen[v] == 1, "vector %zu (row %zu, group %zu) not visited", v, v / G, v % G);
    for (uint32_t y = 0; y < rows; y++)
        CHECK(row_piece[y] != 0xff && (y == 0 || row_piece[y] >= row_piece[y - 1]), "row %u: pieces out of order", y);
    printf("%u %u %u %d %u %u %u %u\n", W, rows, grid, (int)slabs, ilp, p0.pieces, p0.B, max_trips);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 6 || (argc - 1) % 5 != 0) {
        fprintf(stderr, "usage: %s (W rows grid slabs ilp)...\n", argv[0]);
        return 2;
    }
    for (int i = 1; i + 4 < argc; i += 5) {
        const uint32_t W = (uint32_t)strtoul(argv[i], nullptr, 10), rows = (uint32_t)strtoul(argv[i + 1], nullptr, 10);
        const uint32_t grid = (uint32_t)strtoul(argv[i + 2], nullptr, 10), ilp = (uint32_t)strtoul(argv[i + 4], nullptr, 10);
        const bool slabs = atoi(argv[i + 3]) != 0;
        if (W % 16u || W < 1040u || !rows || !grid || !ilp) {
            fprintf(stderr, "bad case %u %u %u %u\n", W, rows, grid, ilp);
            return 2;
        }
        if (walk(W, rows, grid, slabs, ilp)) {
            fprintf(stderr, "case W=%u rows=%u grid=%u slabs=%d ilp=%u\n", W, rows, grid, (int)slabs, ilp);
            return 1;
        }
    }
    return 0;
}
