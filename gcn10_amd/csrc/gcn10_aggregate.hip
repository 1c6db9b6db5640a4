// gcn10_aggregate.hip -- area-mean CN rasters on a coarser grid (config key aggregate=<f>, DESIGN.md "Aggregated
// rasters").
//
// Cell (cx, cy) of the output is the mean of raster r over the f x f landcover pixels from column x0 + cx f and row
// cy f on (clipped at x1 and at the strip's last row), the value 255 left out: (2 s + n) / (2 n), rounded half up,
// 255 when n = 0 -- the rule of the average overviews (gcn10_overview.hip).  No full-resolution CN raster is made:
// the kernels read what cn_strip reads, a landcover strip and the soil code bytes of the prepared tile.
//
// A workgroup owns one cell row and a chunk of its cells, stages the all-tables image once and keeps one pair of
// LDS words per (raster, cell): the sum of ALL the footprint's bytes and the number of its 255 bytes.  From those,
// s = sum - 255 n255 and n = footprint - n255, the footprint being known from the geometry alone.  No cell belongs to
// two workgroups or two calls, so there are no global atomics and the result does not depend on the launch shape.
//
// The unit of work is a 16-pixel column group of the soil rows (the soil load is aligned, the landcover load is
// not, as in the pair histograms).  gather16 gives four pixels of one raster per dword, so "the pixels of this
// group that belong to cell c" is a byte mask per dword, the same for every row of the cell row:
//
//   f >= 16  aggregate_kernel: a group meets at most two cells, A and B.  A lane takes one group, walks the cell
//            row's rows with the next row's loads in flight, and keeps the 18 x 2 x 2 partial sums in registers
//            (v_dot4_u32_u8 against a mask of 0 / 1 bytes adds the cell's bytes, and likewise its 255 flags); one
//            round of LDS adds per lane at the end, then the division pass.
//   f < 16   aggregate_small_kernel: a group meets up to nine cells.  The work items are (group, row) pairs dealt to
//            the lanes, and every cell of an item is added to LDS directly.  This is the slow form for the factors
//            nobody aggregates a 10 m grid by; it shares everything but the accumulation.
//
// Pixels outside [px_lo, px_hi) -- the chunk's own columns -- are masked out, so a group that two chunks share is
// read by both and counted by each for its own cells only; pixels at or beyond W are never read.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gcn10_gpu_internal.hpp"
#include "gcn10_soil_readers.hpp"

using namespace gcn10;

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kPxPerLane = 16;
constexpr uint32_t kMinFactor = 2, kMaxFactor = 256;
// cells of a chunk at most: the cells that 256 groups less one (the chunk starts anywhere in its first group) hold
// at f = 16.  The LDS words of a chunk's cells are dynamic shared memory, 2 x 18 x cells_per_chunk of them: [sum |
// n255][raster][cell].
constexpr uint32_t kMaxCells = (kThreads * kPxPerLane - kPxPerLane) / 16u;        // 255

struct AggParams {
    const uint8_t *esa;         // strip, W x rows, row major
    SoilView soil;              // soil code bytes, soil row of every strip row
    const uint8_t *lut16;
    uint32_t W, rows, x0, x1, f;
    uint32_t Wa, cells_per_chunk, chunks;
    uint32_t sel;               // bit r: raster r is selected
    size_t out_stride;
    uint8_t *out[GCN10_N_RASTERS];
};

typedef u32x4 u32x4_u __attribute__((aligned(1)));

__device__ __forceinline__ uint8_t avg_of(uint32_t s, uint32_t n)
{
    return n == 0 ? (uint8_t)GCN10_NODATA : (uint8_t)((2u * s + n) / (2u * n));
}

// 0x80 in every byte of v that is 255
__device__ __forceinline__ uint32_t ff_bytes(uint32_t v)
{
    return ((v & 0x7f7f7f7fu) + 0x01010101u) & v & 0x80808080u;
}

// 0xff in bytes [a, b) of dword j of a lane's 16 pixels, a <= b <= 16
__device__ __forceinline__ uint32_t range_mask(uint32_t j, uint32_t a, uint32_t b)
{
    const uint32_t lo = min(max(a, 4u * j), 4u * j + 4u) - 4u * j;
    const uint32_t hi = min(max(b, 4u * j), 4u * j + 4u) - 4u * j;
    const uint64_t m = ((1ull << (8u * hi)) - 1ull) & ~((1ull << (8u * lo)) - 1ull);
    return (uint32_t)m;
}

// the same with 0x01 per byte: what v_dot4_u32_u8 multiplies a cell's bytes by
__device__ __forceinline__ uint32_t range_ones(uint32_t j, uint32_t a, uint32_t b)
{
    return range_mask(j, a, b) & 0x01010101u;
}

// The bytes of v that `ones` selects added to s, and 128 for each of them that is 255 (ff = ff_bytes(v)) to n128:
// one v_dot4_u32_u8 each.  A lane adds at most 256 rows x 16 pixels, so n128 stays below 2^20.
__device__ __forceinline__ void add_bytes(uint32_t v, uint32_t ff, uint32_t ones, uint32_t &s, uint32_t &n128)
{
    s = __builtin_amdgcn_udot4(v, ones, s, false);
    n128 = __builtin_amdgcn_udot4(ff, ones, n128, false);
}

// 16 landcover and 16 soil bytes of the group at column gx of strip row y; the pixels at or beyond W read as zero
// and are not touched (the soil rows are padded beyond W, the landcover is not)
__device__ __forceinline__ void load_group(const AggParams &p, uint32_t y, uint32_t gx, u32x4 &e, u32x4 &c)
{
    const uint8_t *erow = p.esa + (size_t)y * p.W + gx;
    c = *reinterpret_cast<const u32x4 *>(p.soil.ptr(y, gx));
    if (gx + kPxPerLane <= p.W) {
        e = *reinterpret_cast<const u32x4_u *>(erow);
    }
    else {
        const uint32_t m = p.W - gx;
        e = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t i = 0; i < kPxPerLane - 1u; i++)     // constant indices: the vector stays in registers
            if (i < m)
                e[i >> 2] |= (uint32_t)erow[i] << (8u * (i & 3u));
#pragma unroll
        for (uint32_t j = 0; j < 4; j++)
            c[j] &= range_mask(j, 0u, m);
    }
}

struct Chunk {
    uint32_t cy, c0, nc;        // cell row, first cell and number of cells
    uint32_t px_lo, px_hi;      // its columns
    uint32_t y_lo, ny;          // its rows of the strip
    uint32_t g0, ng;            // first group (in groups of 16 columns) and number of groups
};

__device__ __forceinline__ Chunk chunk_of(const AggParams &p)
{
    Chunk k;
    k.cy = blockIdx.x / p.chunks;
    k.c0 = (blockIdx.x - k.cy * p.chunks) * p.cells_per_chunk;
    k.nc = min(p.cells_per_chunk, p.Wa - k.c0);
    k.px_lo = p.x0 + k.c0 * p.f;
    k.px_hi = min(k.px_lo + k.nc * p.f, p.x1);
    k.y_lo = k.cy * p.f;
    k.ny = min(p.f, p.rows - k.y_lo);
    k.g0 = k.px_lo >> 4;
    k.ng = ((k.px_hi - 1u) >> 4) - k.g0 + 1u;
    return k;
}

// the division pass: raster after raster, so that neighbouring lanes store neighbouring bytes
__device__ __forceinline__ void store_cells(const AggParams &p, const Chunk &k, const uint32_t *sum,
                                            const uint32_t *n255)
{
    const uint32_t cpc = p.cells_per_chunk;
    for (uint32_t r = 0; r < GCN10_N_RASTERS; r++) {
        if (!(p.sel & (1u << r)))
            continue;
        uint8_t *o = p.out[r] + (size_t)k.cy * p.out_stride + k.c0;
        for (uint32_t c = threadIdx.x; c < k.nc; c += kThreads) {
            const uint32_t left = k.px_lo + c * p.f;
            const uint32_t area = (min(left + p.f, p.x1) - left) * k.ny;
            const uint32_t nff = n255[r * cpc + c];
            o[c] = avg_of(sum[r * cpc + c] - 255u * nff, area - nff);
        }
    }
}

// ---- f >= 16 ------------------------------------------------------------------------------------------------------
template <int C>
__device__ __forceinline__ void add_cond(const AggParams &p, const uint8_t *lut, const u32x4 &e, const u32x4 &c,
                                         const uint32_t (&ma)[4], const uint32_t (&mb)[4],
                                         uint32_t (&sa)[GCN10_N_RASTERS], uint32_t (&na)[GCN10_N_RASTERS],
                                         uint32_t (&sb)[GCN10_N_RASTERS], uint32_t (&nb)[GCN10_N_RASTERS])
{
    if (!((p.sel >> (9 * C)) & 0x1ffu))
        return;
    uint32_t acc[9][4];
    gather16(lut, e, c, C, acc);
#pragma unroll
    for (int t = 0; t < 9; t++) {
        const int r = C * 9 + t;
        if (!(p.sel & (1u << r)))
            continue;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t v = acc[t][j], ff = ff_bytes(v);
            add_bytes(v, ff, ma[j], sa[r], na[r]);
            add_bytes(v, ff, mb[j], sb[r], nb[r]);
        }
    }
}

__global__ __launch_bounds__(kThreads) void aggregate_kernel(const AggParams p)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[kLut16Bytes];
    extern __shared__ uint32_t cell_words[];
    const uint32_t cpc = p.cells_per_chunk;
    uint32_t *const sum = cell_words, *const n255 = cell_words + GCN10_N_RASTERS * cpc;
    stage_lut16<kThreads>(lut, p.lut16);
    for (uint32_t i = threadIdx.x; i < 2u * GCN10_N_RASTERS * cpc; i += kThreads)
        cell_words[i] = 0u;
    __syncthreads();

    const Chunk k = chunk_of(p);
    // ng <= kThreads by the choice of cells_per_chunk; the loop is for the reader
    for (uint32_t g = threadIdx.x; g < k.ng; g += kThreads) {
        const uint32_t gx = (k.g0 + g) << 4;
        const uint32_t a = max(gx, k.px_lo), b = min(gx + kPxPerLane, k.px_hi);    // a < b: the group meets the chunk
        const uint32_t ca = (a - p.x0) / p.f;                           // cell A, and where cell B begins
        const uint32_t edge = min(p.x0 + (ca + 1u) * p.f, b);
        uint32_t ma[4], mb[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            ma[j] = range_ones(j, a - gx, edge - gx);
            mb[j] = range_ones(j, edge - gx, b - gx);
        }
        uint32_t sa[GCN10_N_RASTERS], na[GCN10_N_RASTERS], sb[GCN10_N_RASTERS], nb[GCN10_N_RASTERS];
#pragma unroll
        for (int r = 0; r < GCN10_N_RASTERS; r++)
            sa[r] = na[r] = sb[r] = nb[r] = 0u;

        u32x4 e, c, e_next, c_next;
        load_group(p, k.y_lo, gx, e, c);
        for (uint32_t j = 0; j < k.ny; j++) {
            // the next row's loads in flight over this row's gathers (the last trip reloads its own row)
            load_group(p, k.y_lo + min(j + 1u, k.ny - 1u), gx, e_next, c_next);
            add_cond<0>(p, lut, e, c, ma, mb, sa, na, sb, nb);
            add_cond<1>(p, lut, e, c, ma, mb, sa, na, sb, nb);
            e = e_next;
            c = c_next;
        }

        const uint32_t la = ca - k.c0;          // < nc, and cell B exists only inside the chunk
        const bool has_b = edge < b;
#pragma unroll
        for (int r = 0; r < GCN10_N_RASTERS; r++) {
            if (!(p.sel & (1u << r)))
                continue;
            atomicAdd(&sum[r * cpc + la], sa[r]);
            if (na[r])
                atomicAdd(&n255[r * cpc + la], na[r] >> 7);
            if (has_b) {
                atomicAdd(&sum[r * cpc + la + 1u], sb[r]);
                if (nb[r])
                    atomicAdd(&n255[r * cpc + la + 1u], nb[r] >> 7);
            }
        }
    }
    __syncthreads();
    store_cells(p, k, sum, n255);
}

// ---- f < 16 -------------------------------------------------------------------------------------------------------
template <int C>
__device__ __forceinline__ void add_cond_small(const AggParams &p, const Chunk &k, const uint8_t *lut, const u32x4 &e,
                                               const u32x4 &c, uint32_t gx, uint32_t a, uint32_t b, uint32_t *sum,
                                               uint32_t *n255)
{
    const uint32_t cpc = p.cells_per_chunk;
    if (!((p.sel >> (9 * C)) & 0x1ffu))
        return;
    uint32_t acc[9][4];
    gather16(lut, e, c, C, acc);
    uint32_t cell = (a - p.x0) / p.f;
    for (uint32_t from = a; from < b; cell++) {
        const uint32_t to = min(p.x0 + (cell + 1u) * p.f, b);
        uint32_t m[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++)
            m[j] = range_ones(j, from - gx, to - gx);
        const uint32_t lc = cell - k.c0;
#pragma unroll
        for (int t = 0; t < 9; t++) {
            const int r = C * 9 + t;
            if (!(p.sel & (1u << r)))
                continue;
            uint32_t s = 0u, n = 0u;
#pragma unroll
            for (int j = 0; j < 4; j++)
                add_bytes(acc[t][j], ff_bytes(acc[t][j]), m[j], s, n);
            atomicAdd(&sum[r * cpc + lc], s);
            if (n)
                atomicAdd(&n255[r * cpc + lc], n >> 7);
        }
        from = to;
    }
}

__global__ __launch_bounds__(kThreads) void aggregate_small_kernel(const AggParams p)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[kLut16Bytes];
    extern __shared__ uint32_t cell_words[];
    const uint32_t cpc = p.cells_per_chunk;
    uint32_t *const sum = cell_words, *const n255 = cell_words + GCN10_N_RASTERS * cpc;
    stage_lut16<kThreads>(lut, p.lut16);
    for (uint32_t i = threadIdx.x; i < 2u * GCN10_N_RASTERS * cpc; i += kThreads)
        cell_words[i] = 0u;
    __syncthreads();

    const Chunk k = chunk_of(p);
    for (uint32_t i = threadIdx.x; i < k.ng * k.ny; i += kThreads) {
        const uint32_t j = i / k.ng, g = i - j * k.ng;
        const uint32_t gx = (k.g0 + g) << 4;
        const uint32_t a = max(gx, k.px_lo), b = min(gx + kPxPerLane, k.px_hi);
        u32x4 e, c;
        load_group(p, k.y_lo + j, gx, e, c);
        add_cond_small<0>(p, k, lut, e, c, gx, a, b, sum, n255);
        add_cond_small<1>(p, k, lut, e, c, gx, a, b, sum, n255);
    }
    __syncthreads();
    store_cells(p, k, sum, n255);
}

}  // namespace

extern "C" {

int gcn10_gpu_aggregate(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj, int x0, int x1,
                        int factor, unsigned cond_mask, unsigned table_mask, uint8_t *const *out, size_t out_stride,
                        gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    const char *const who = "gcn10_gpu_aggregate";
    hipStream_t s = as_stream(ctx, stream);
    AggParams p = {};
    if ((rc = check_tables(ctx, who)) != GCN10_OK || (rc = bind_soil(ctx, who, W, s, cj, &p.soil)) != GCN10_OK)
        return rc;
    if (!esa || !cj || !out || W <= 0 || rows <= 0 || factor < (int)kMinFactor || factor > (int)kMaxFactor || x0 < 0 ||
        x0 >= x1 || x1 > W)
        return fail(GCN10_E_INVAL, "gcn10_gpu_aggregate: bad arguments W=%d rows=%d columns [%d, %d) factor=%d "
                    "(factor 2..256, 0 <= x0 < x1 <= W)", W, rows, x0, x1, factor);
    if ((rc = check_masks(ctx, who, cond_mask, table_mask)) != GCN10_OK)
        return rc;
    p.esa = esa;
    p.lut16 = ctx->d_lut16;
    p.W = (uint32_t)W;
    p.rows = (uint32_t)rows;
    p.x0 = (uint32_t)x0;
    p.x1 = (uint32_t)x1;
    p.f = (uint32_t)factor;
    p.Wa = (p.x1 - p.x0 + p.f - 1u) / p.f;
    if (out_stride < p.Wa)
        return fail(GCN10_E_INVAL, "gcn10_gpu_aggregate: out_stride %zu for rows of %u cells", out_stride, p.Wa);
    p.out_stride = out_stride;
    int q = 0;
    for (int r = 0; r < GCN10_N_RASTERS; r++) {
        if (!selected((uint32_t)r, cond_mask, table_mask))
            continue;
        if (!out[q])
            return fail(GCN10_E_INVAL, "gcn10_gpu_aggregate: output %d (raster %d) is NULL", q, r);
        p.out[r] = out[q++];
        p.sel |= 1u << r;
    }
    // f >= 16: as many cells as 255 groups hold, so that a chunk starting anywhere in its first group has at most
    // 256 groups, one per lane.  f < 16: all the cells the LDS words hold.
    const bool small = p.f < kPxPerLane;
    p.cells_per_chunk = small ? kMaxCells : (kThreads * kPxPerLane - kPxPerLane) / p.f;
    p.chunks = (p.Wa + p.cells_per_chunk - 1u) / p.cells_per_chunk;
    const uint64_t grid = (uint64_t)((p.rows + p.f - 1u) / p.f) * p.chunks;
    if (grid > 0x7fffffffull)
        return fail(GCN10_E_INVAL, "gcn10_gpu_aggregate: %llu workgroups; cut the strip into bands",
                    (unsigned long long)grid);
    const size_t cell_bytes = 2u * GCN10_N_RASTERS * (size_t)p.cells_per_chunk * sizeof(uint32_t);
    hipLaunchKernelGGL(small ? aggregate_small_kernel : aggregate_kernel, dim3((uint32_t)grid), dim3(kThreads),
                       cell_bytes, s, p);
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}

}  // extern "C"
