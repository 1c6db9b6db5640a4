// gcn10_grid.hip -- sums of every selected raster over the cells of a model grid (config key grid=..., DESIGN.md
// "Model grid").
//
// The cells are given by two maps, the local cell column of every pixel column and the local cell row of every strip
// row (-1: in no cell), made on the host from coordinates (host/grid.c): cells are no whole number of pixels, they
// differ by a pixel from one to the next, and a cell can be wider than a workgroup's columns or taller than its rows.
// gcn10_gpu_grid_sums ADDS the sum and the count of the values != 255 of every cell to 64-bit pairs in global memory;
// gcn10_gpu_grid_finish turns pairs into bytes by the rule of the area means, (2 s + n) / (2 n), 255 when n = 0.  No
// full-resolution CN raster is made: the kernel reads what gcn10_gpu_aggregate reads, a landcover strip and the soil
// code bytes of the prepared tile.
//
// A workgroup takes one drainage condition (the nine rasters of it), 256 column groups of 16 pixels and a band of the
// strip's rows, a lane one group.  The non-negative entries of a map never decrease, and with cells of 8 pixels or
// more a group meets at most three cell columns; which of its pixels belong to the first, second and third of them is
// a mask of 0 / 1 bytes per dword that holds for every row, so the v_dot4_u32_u8 sums of the area means carry over
// with a third mask (skipped by the waves none of whose groups has a third, or a second, cell).  The lane keeps 9 x 3
// x 2 partial sums in registers while the cell row stays the same -- the row is the same for the whole workgroup, so
// that is a uniform test --, then adds them to the workgroup's LDS words per (raster, cell column), and the workgroup
// issues ONE pair of 64-bit atomic adds per (raster, cell) it has met: never one per pixel, lane or wave.  Small cells:
// a band holds several cell rows and only the cell rows cut by a band's first and last row get adds from two
// workgroups.  Large cells: the bands split a cell's rows over many workgroups so that the device is filled.  Only
// integers are added, so the pairs do not depend on bands, chunks or order.
//
// Nothing at or beyond W is read (the last group of a row is read byte by byte, as in the area means); map entries
// outside [0, ncx) and [0, ncy) count as -1, and a cell column beyond the kMaxCells a chunk's LDS words hold is left
// out, so no map makes the kernel write outside acc.
//
// Weighted sums (DESIGN.md "Runoff-weighted composites", "Several storms"): with k tables w_j of 256 16-bit weights a
// (raster, cell) has 2 + k words, word 2 + j the sum of w_j[v] over the same pixels.  w o table is a function of (soil
// plane, landcover, table) like the value itself, so gcn10_gpu_set_weight_tables folds every w_j into two more images
// of the all-tables layout, the low and the high bytes of w_j[cn], zero where the CN image holds 255; against such an
// image the same gather, masks and dot products give the sum of the low and of the high bytes, and sw = lo + 256 hi.
// In a weight plane 255 is a number: a plane pass makes no 255 test and no count.  A workgroup keeps its shape and
// gets a role besides its condition, one of 1 + 2 k -- the CN image (words 0 and 1), then (low, high) of table 0, 1,
// ...: word 2 + j, the high plane's sums shifted by 8 --, and the workgroups of an item are dealt to one XCD.  The word
// count and a plane role's target word are uniform run-time values that enter only the addresses of the flush's
// atomics; a plane role stages one image, so the LDS of a workgroup does not depend on k.  The finish pass keeps
// k x 101 weights in LDS and decides per table between bisection and the scan from 1.
//
// ONE sums kernel and ONE finish kernel serve all three pairs of calls: gcn10_gpu_grid_sums / _finish are k = 0
// whatever weights the context holds (pairs, one role, no plane and no weight is touched), the _weighted calls are
// k = 1 (gcn10_gpu_set_weights is gcn10_gpu_set_weight_tables with one table), the _storms calls the context's k.
// The sums kernel has two instantiations, k at run time and k = 0 at compile time, picked from k in its one launch.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "gcn10_grid_internal.hpp"

using namespace gcn10;

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kPxPerLane = 16;
constexpr uint32_t kChunkPx = kThreads * kPxPerLane;        // 4096 columns of a workgroup
// cell columns of a chunk at most: 4096 / 8 whole ones and a cut one at either end.  The LDS words of a chunk: the sum
// of ALL bytes and the number of 255 bytes per (raster of the condition, cell), and the pixels per cell.
constexpr uint32_t kMaxCells = kChunkPx / 8u + 2u;          // 514
constexpr uint32_t kMaxBandRows = 256;                      // a lane's and a chunk's 32-bit sums hold 4096 x 256 x 255
constexpr uint32_t kNoCell = 0xffffffffu;

struct GridParams {
    const uint8_t *esa;         // strip, W x rows, row major
    SoilView soil;              // soil code bytes, soil row of every strip row
    const uint8_t *image;       // the CN image
    const int32_t *cellx, *celly;
    uint32_t W, rows, ncx, ncy;
    uint32_t chunks, band_rows;
    uint32_t items;             // chunks x bands
    uint32_t sel;               // bit r: raster r is selected
    uint32_t n_conds, conds[2]; // the selected conditions
    uint32_t k;                 // tables of weights, 0 to GCN10_GPU_MAX_WEIGHT_TABLES
    unsigned long long *acc;    // [n_sel][ncy][ncx][2 + k]
    const uint8_t *planes;      // [2 k] images: the low and the high plane of table 0, of table 1, ...
};

// the LDS of a workgroup: 62.3 KiB
struct GridLds {
    __attribute__((aligned(16))) uint8_t lut[kLut16Bytes];
    uint32_t sum[9 * kMaxCells], n255[9 * kMaxCells], area[kMaxCells];
    uint32_t cell_lo, cell_hi;
};

// 0x80 in every byte of v that is 255
__device__ __forceinline__ uint32_t ff_bytes(uint32_t v)
{
    return ((v & 0x7f7f7f7fu) + 0x01010101u) & v & 0x80808080u;
}

// 0xff in bytes [0, m) of dword j of a lane's 16 pixels
__device__ __forceinline__ uint32_t head_mask(uint32_t j, uint32_t m)
{
    const uint32_t hi = min(max(m, 4u * j), 4u * j + 4u) - 4u * j;
    return (uint32_t)((1ull << (8u * hi)) - 1ull);
}

// 16 landcover and 16 soil bytes of the group at column gx of strip row y; the pixels at or beyond W read as zero and
// are not touched (the soil rows are padded beyond W, the landcover is not)
__device__ __forceinline__ void load_group(const GridParams &p, uint32_t y, uint32_t gx, u32x4 &e, u32x4 &c)
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
            c[j] &= head_mask(j, m);
    }
}

// The sums of one row: the nine rasters' four dwords against the masks of the lane's first cell, and of its second
// (has_b) and third (has_c) where some lane of the wave has one: straight-line code per case, no branch per dword.
// PLANE: the image is a weight plane -- every byte is a number, nothing is counted.
template <bool PLANE, bool has_b, bool has_c>
__device__ __forceinline__ void add_row(const uint8_t *lut, const u32x4 &e, const u32x4 &c, uint32_t cond,
                                        uint32_t sel9, const uint32_t (&m)[3][4], uint32_t (&s)[3][9],
                                        uint32_t (&n)[3][9])
{
    uint32_t acc[9][4];
    gather16(lut, e, c, (int)cond, acc);
#pragma unroll
    for (int t = 0; t < 9; t++) {
        if (!(sel9 & (1u << t)))
            continue;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t v = acc[t][j], ff = PLANE ? 0u : ff_bytes(v);
            s[0][t] = __builtin_amdgcn_udot4(v, m[0][j], s[0][t], false);
            if (!PLANE)
                n[0][t] = __builtin_amdgcn_udot4(ff, m[0][j], n[0][t], false);
            if (has_b) {
                s[1][t] = __builtin_amdgcn_udot4(v, m[1][j], s[1][t], false);
                if (!PLANE)
                    n[1][t] = __builtin_amdgcn_udot4(ff, m[1][j], n[1][t], false);
            }
            if (has_c) {
                s[2][t] = __builtin_amdgcn_udot4(v, m[2][j], s[2][t], false);
                if (!PLANE)
                    n[2][t] = __builtin_amdgcn_udot4(ff, m[2][j], n[2][t], false);
            }
        }
    }
}

// One workgroup's item (chunk, band) for condition `cond`.  PLANE = false: against the CN image, words 0 and 1 of
// `words` per (raster, cell).  PLANE = true: against the weight plane `image`, its sums shifted by `shift` into word
// `plane_word`.  Both are uniform run-time values that enter the addresses of the flush's atomics only.
template <bool PLANE>
__device__ __forceinline__ void sum_item(const GridParams &p, GridLds &lds, const uint32_t item, const uint32_t cond,
                                         const uint8_t *image, const uint32_t shift, const uint32_t words,
                                         const uint32_t plane_word)
{
    uint8_t *const lut = lds.lut;
    uint32_t *const sum = lds.sum, *const n255 = lds.n255, *const area = lds.area;
    uint32_t &cell_lo = lds.cell_lo, &cell_hi = lds.cell_hi;
    const uint32_t sel9 = (p.sel >> (9u * cond)) & 0x1ffu;
    const uint32_t band = item / p.chunks;
    const uint32_t gx = (item - band * p.chunks) * kChunkPx + threadIdx.x * kPxPerLane;
    const uint32_t y_lo = band * p.band_rows, y_hi = min(y_lo + p.band_rows, p.rows);

    stage_lut16<kThreads>(lut, image);
    for (uint32_t i = threadIdx.x; i < 9u * kMaxCells; i += kThreads)
        sum[i] = n255[i] = 0u;
    for (uint32_t i = threadIdx.x; i < kMaxCells; i += kThreads)
        area[i] = 0u;
    if (threadIdx.x == 0) {
        cell_lo = kNoCell;
        cell_hi = 0u;
    }
    __syncthreads();

    // the lane's cells: the first three different values of its 16 columns, and their masks
    uint32_t cell[3] = {kNoCell, kNoCell, kNoCell};
    uint32_t m[3][4] = {};
    uint32_t px[3] = {0u, 0u, 0u};
#pragma unroll
    for (uint32_t i = 0; i < kPxPerLane; i++) {
        const uint32_t x = gx + i;
        const uint32_t c = x < p.W ? (uint32_t)p.cellx[x] : kNoCell;       // a negative entry is >= ncx
        if (c >= p.ncx)
            continue;
        const uint32_t k = cell[0] == kNoCell || cell[0] == c ? 0u
                         : cell[1] == kNoCell || cell[1] == c ? 1u
                         : cell[2] == kNoCell || cell[2] == c ? 2u : 3u;
#pragma unroll
        for (uint32_t kk = 0; kk < 3; kk++)
            if (k == kk) {
                cell[kk] = c;
                m[kk][i >> 2] |= 1u << (8u * (i & 3u));
                px[kk]++;
            }
    }
    if (cell[0] != kNoCell) {
        atomicMin(&cell_lo, cell[0]);
        atomicMax(&cell_hi, cell[2] != kNoCell ? cell[2] : cell[1] != kNoCell ? cell[1] : cell[0]);
    }
    __syncthreads();
    const uint32_t c_lo = cell_lo;
    if (c_lo == kNoCell)
        return;                 // no column of the chunk is in a cell (the same for the whole workgroup)
    const uint32_t n_cells = min(cell_hi - c_lo + 1u, kMaxCells);
    // local cells; one beyond the LDS words (a map that breaks the rule of 8 pixels per cell) is left out
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) {
        if (cell[k] != kNoCell && cell[k] - c_lo >= kMaxCells) {
            cell[k] = kNoCell;
#pragma unroll
            for (uint32_t j = 0; j < 4; j++)
                m[k][j] = 0u;
        }
        if (cell[k] != kNoCell)
            cell[k] -= c_lo;
    }
    const bool active = cell[0] != kNoCell || cell[1] != kNoCell || cell[2] != kNoCell;
    const bool has_b = __any(cell[1] != kNoCell), has_c = __any(cell[2] != kNoCell);

    uint32_t s[3][9], n[3][9];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int t = 0; t < 9; t++)
            s[k][t] = n[k][t] = 0u;

    uint32_t cur = kNoCell, seg_rows = 0u;      // the cell row of the rows added up so far, and how many they are
    u32x4 e = {}, c = {}, e_next = {}, c_next = {};
    if (active)
        load_group(p, y_lo, gx, e, c);
    for (uint32_t y = y_lo; y <= y_hi; y++) {
        uint32_t cy = kNoCell;
        if (y < y_hi) {
            cy = (uint32_t)p.celly[y];
            if (cy >= p.ncy)
                cy = kNoCell;
        }
        if (cy != cur && cur != kNoCell) {
            // the cell row ends: registers -> LDS, then one pair of atomics per (raster, cell) of the chunk
            if (active) {
#pragma unroll
                for (uint32_t k = 0; k < 3; k++) {
                    if (cell[k] == kNoCell)
                        continue;
                    if (!PLANE)
                        atomicAdd(&area[cell[k]], px[k] * seg_rows);
#pragma unroll
                    for (uint32_t t = 0; t < 9; t++) {
                        if (!(sel9 & (1u << t)))
                            continue;
                        atomicAdd(&sum[t * kMaxCells + cell[k]], s[k][t]);
                        if (!PLANE && n[k][t])
                            atomicAdd(&n255[t * kMaxCells + cell[k]], n[k][t] >> 7);
                        s[k][t] = n[k][t] = 0u;
                    }
                }
            }
            __syncthreads();
            if (PLANE) {
                // one lane per cell: the plane's sum of every raster, shifted, to its word
                for (uint32_t lc = threadIdx.x; lc < n_cells; lc += kThreads) {
                    for (uint32_t t = 0; t < 9; t++) {
                        if (!(sel9 & (1u << t)))
                            continue;
                        const uint32_t q = __popc(p.sel & ((1u << (9u * cond + t)) - 1u));
                        const uint32_t sv = sum[t * kMaxCells + lc];
                        sum[t * kMaxCells + lc] = 0u;
                        if (sv)
                            atomicAdd(p.acc + ((((size_t)q * p.ncy + cur) * p.ncx + c_lo + lc) * words + plane_word),
                                      (unsigned long long)sv << shift);
                    }
                }
            }
            else {
                // lanes 2i and 2i + 1 add s and n of cell i: a wave's adds are 512 contiguous bytes (with k tables:
                // two words of every 2 + k)
                for (uint32_t i = threadIdx.x; i < 2u * n_cells; i += kThreads) {
                    const uint32_t lc = i >> 1, word = i & 1u;
                    const uint32_t a = area[lc];
                    for (uint32_t t = 0; t < 9; t++) {
                        if (!(sel9 & (1u << t)))
                            continue;
                        const uint32_t q = __popc(p.sel & ((1u << (9u * cond + t)) - 1u));
                        const uint32_t nff = n255[t * kMaxCells + lc];
                        const uint32_t sv = sum[t * kMaxCells + lc] - 255u * nff, nv = a - nff;
                        sum[t * kMaxCells + lc] = 0u;
                        n255[t * kMaxCells + lc] = 0u;
                        if (nv)
                            atomicAdd(p.acc + ((((size_t)q * p.ncy + cur) * p.ncx + c_lo + lc) * words + word),
                                      (unsigned long long)(word ? nv : sv));
                    }
                    area[lc] = 0u;
                }
            }
            __syncthreads();
            seg_rows = 0u;
        }
        cur = cy;
        if (y >= y_hi)
            break;
        if (active) {
            // the next row's loads in flight over this row's gathers (the last trip reloads its own row)
            load_group(p, min(y + 1u, y_hi - 1u), gx, e_next, c_next);
            if (cy != kNoCell) {
                if (has_c)
                    add_row<PLANE, true, true>(lut, e, c, cond, sel9, m, s, n);
                else if (has_b)
                    add_row<PLANE, true, false>(lut, e, c, cond, sel9, m, s, n);
                else
                    add_row<PLANE, false, false>(lut, e, c, cond, sel9, m, s, n);
            }
            e = e_next;
            c = c_next;
        }
        seg_rows += cy != kNoCell ? 1u : 0u;
    }
}

// With R roles per item -- the conditions, times 1 + 2 k with k tables -- workgroups j, j + 8, ..., j + 8 (R - 1) of
// every 8 R take the roles of one item (chunk, band): consecutive workgroups go to the eight XCDs in turn, so the
// workgroups that read the same landcover and soil run on the same XCD at about the same time, and its L2 has what
// the later ones read.  The last 8 R are padded.
__device__ __forceinline__ bool deal_item(const GridParams &p, uint32_t roles, uint32_t &item, uint32_t &role)
{
    item = blockIdx.x;
    role = 0u;
    if (roles > 1u) {
        const uint32_t group = blockIdx.x / (8u * roles), in = blockIdx.x - group * (8u * roles);
        item = group * 8u + (in & 7u);
        role = in >> 3;
    }
    return item < p.items;      // the same for the whole workgroup
}

// Roles of an item: (condition, image), the 1 + 2 k images of a condition next to each other -- the CN image, then
// (low, high) of table 0, 1, ...  TABLES = false is the same kernel with k a compile-time 0: measured, the plain call
// is 1.5 % slower at cells of 25 px with k = 0 at run time (DESIGN.md "Model grid").
template <bool TABLES>
__global__ __launch_bounds__(kThreads) void grid_sums_kernel(const GridParams p)
{
    __shared__ GridLds lds;
    const uint32_t k = TABLES ? p.k : 0u, per = 1u + 2u * k, words = 2u + k;
    uint32_t item, role;
    if (!deal_item(p, per * p.n_conds, item, role))
        return;
    const uint32_t cond = p.conds[role / per], image = role % per;
    if (image == 0u)
        sum_item<false>(p, lds, item, cond, p.image, 0u, words, 0u);
    else
        sum_item<true>(p, lds, item, cond, p.planes + (size_t)(image - 1u) * kLut16Bytes, (image & 1u) ? 0u : 8u,
                       words, 2u + ((image - 1u) >> 1));
}

struct FinishParams {
    const unsigned long long *acc;
    size_t n_cells, total;      // cells per raster, and over all rasters
    uint8_t *means, *cnq;       // cnq: [k][n_sel][n_cells]
    const uint32_t *shared_idx;
    uint32_t n_shared, n_sel;
    unsigned long long *shared;
    const uint16_t *weights;    // [k][256]: the context's, on the device
    uint32_t rising;            // bit j: weights[j][1..100] never decrease
    uint32_t k;
};

// 2 + k words per (raster, cell): the means, k runoff-equivalent bytes per cell and the shared cells' 2 + k words
__global__ __launch_bounds__(kThreads) void grid_finish_kernel(const FinishParams p)
{
    __shared__ uint32_t w[GCN10_GPU_MAX_WEIGHT_TABLES * 101];
    const uint32_t k = p.k, words = 2u + k;
    for (uint32_t i = threadIdx.x; i < k * 101u; i += kThreads)
        w[i] = p.weights[(i / 101u) * 256u + i % 101u];
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < p.total; i += stride) {
        const unsigned long long s = p.acc[words * i], n = p.acc[words * i + 1u];
        p.means[i] = mean_byte(s, n);
        for (uint32_t j = 0; j < k; j++) {
            const unsigned long long sw = p.acc[words * i + 2u + j];
            // two copies of the rule: each has one of its loops only
            p.cnq[(size_t)j * p.total + i] = (p.rising >> j) & 1u ? runoff_cn(w + 101u * j, true, s, n, sw)
                                                                  : runoff_cn(w + 101u * j, false, s, n, sw);
        }
    }
    const size_t packed = (size_t)p.n_sel * p.n_shared;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < packed; i += stride) {
        const size_t q = i / p.n_shared, c = i - q * p.n_shared;
        const size_t at = q * p.n_cells + p.shared_idx[c];
        for (uint32_t word = 0; word < words; word++)
            p.shared[words * i + word] = p.acc[words * at + word];
    }
}

enum SumsKind { kPlain, kWeighted, kStorms };      // the three pairs of calls, as check_weights words its refusals

// the weights a weighted or a storms call needs: E_STATE without them, and for the one-table calls with several
int check_weights(gcn10_gpu_ctx *ctx, const char *who, SumsKind kind)
{
    if (kind == kPlain)
        return GCN10_OK;
    if (!ctx->weights_set)
        return fail(GCN10_E_STATE, kind == kStorms
                    ? "%s: call gcn10_gpu_set_weight_tables (or gcn10_gpu_set_weights) first (after gcn10_gpu_set_tables)"
                    : "%s: call gcn10_gpu_set_weights first (after gcn10_gpu_set_tables)", who);
    if (kind == kWeighted && ctx->n_weights != 1)
        return fail(GCN10_E_STATE, "%s: the context has %d weight tables; call %s", who, ctx->n_weights,
                    strstr(who, "finish") ? "gcn10_gpu_grid_finish_storms" : "gcn10_gpu_grid_sums_storms");
    return GCN10_OK;
}

// the tables of a call that check_weights has let through: none for the plain calls, WHATEVER the context holds
uint32_t tables_of(const gcn10_gpu_ctx *ctx, SumsKind kind)
{
    return kind == kPlain ? 0u : (uint32_t)ctx->n_weights;
}

int launch_sums(gcn10_gpu_ctx *ctx, const char *who, SumsKind kind, const uint8_t *esa, int W, int rows,
                const int32_t *cj, const int32_t *cellx, const int32_t *celly, int ncx, int ncy, unsigned cond_mask,
                unsigned table_mask, unsigned long long *acc, gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    hipStream_t s = as_stream(ctx, stream);
    GridParams p = {};
    if ((rc = check_tables(ctx, who)) != GCN10_OK)
        return rc;
    if ((rc = check_weights(ctx, who, kind)) != GCN10_OK)
        return rc;
    if ((rc = bind_soil(ctx, who, W, s, cj, &p.soil)) != GCN10_OK)
        return rc;
    if ((rc = check_sums_args(who, esa, W, rows, cj, cellx, celly, ncx, ncy, acc)) != GCN10_OK)
        return rc;
    if ((rc = check_masks(ctx, who, cond_mask, table_mask)) != GCN10_OK)
        return rc;
    p.esa = esa;
    p.image = ctx->d_lut16;
    p.k = tables_of(ctx, kind);
    p.planes = p.k ? ctx->d_wlut : nullptr;
    p.cellx = cellx;
    p.celly = celly;
    p.W = (uint32_t)W;
    p.rows = (uint32_t)rows;
    p.ncx = (uint32_t)ncx;
    p.ncy = (uint32_t)ncy;
    p.acc = acc;
    p.sel = select_rasters(cond_mask, table_mask, p.conds, p.n_conds);
    const uint32_t roles = (1u + 2u * p.k) * p.n_conds;
    p.chunks = (p.W + kChunkPx - 1u) / kChunkPx;
    p.band_rows = band_height(ctx, 8, p.chunks * roles, p.rows, 16u, kMaxBandRows);
    const uint64_t items = (uint64_t)((p.rows + p.band_rows - 1u) / p.band_rows) * p.chunks;
    const uint64_t grid = roles > 1u ? (items + 7u) / 8u * (8u * roles) : items;
    if (grid > 0x7fffffffull)
        return fail(GCN10_E_INVAL, "%s: %llu workgroups; cut the strip into bands", who, (unsigned long long)grid);
    p.items = (uint32_t)items;
    const auto kernel = p.k ? grid_sums_kernel<true> : grid_sums_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)grid), dim3(kThreads), 0, s, p);
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}

int launch_finish(gcn10_gpu_ctx *ctx, const char *who, SumsKind kind, const unsigned long long *acc, int n_sel,
                  size_t n_cells, uint8_t *means, uint8_t *cnq, const uint32_t *shared_idx, uint32_t n_shared,
                  unsigned long long *shared, gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    hipStream_t s = as_stream(ctx, stream);
    if ((rc = check_weights(ctx, who, kind)) != GCN10_OK)
        return rc;
    FinishParams p = {};
    p.k = tables_of(ctx, kind);
    rc = check_finish_args(who, acc, n_sel, n_cells, means, shared_idx, n_shared, shared, !p.k || cnq);
    if (rc != GCN10_OK)
        return rc;
    p.acc = acc;
    p.n_cells = n_cells;
    p.total = n_cells * (size_t)n_sel;
    p.means = means;
    p.cnq = cnq;
    p.shared_idx = shared_idx;
    p.n_shared = n_shared;
    p.n_sel = (uint32_t)n_sel;
    p.shared = shared;
    p.weights = p.k ? reinterpret_cast<const uint16_t *>(ctx->d_wlut + 2 * p.k * kLut16Bytes) : nullptr;
    p.rising = ctx->weights_rising;
    const uint32_t grid = stream_grid(ctx, (p.total + kThreads - 1u) / kThreads);
    hipLaunchKernelGGL(grid_finish_kernel, dim3(grid), dim3(kThreads), 0, s, p);
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}

// k tables of 256 weights into the context: 2 k planes of the loaded tables, then the tables themselves
int fold_weights(gcn10_gpu_ctx *ctx, const char *who, const uint16_t *w, int k)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if ((rc = check_tables(ctx, who)) != GCN10_OK)
        return rc;
    if (!w || k < 1 || k > GCN10_GPU_MAX_WEIGHT_TABLES)
        return fail(GCN10_E_INVAL, "%s: bad arguments k=%d (1..%d tables, no null weights)", who, k,
                    GCN10_GPU_MAX_WEIGHT_TABLES);
    // the CN image as the device holds it, folded: a byte of 255 (no value, padding, a table not loaded) weighs 0
    const size_t table_bytes = 256 * sizeof(uint16_t), planes_bytes = (size_t)k * (2 * kLut16Bytes + table_bytes);
    uint8_t *const img = static_cast<uint8_t *>(malloc(kLut16Bytes + planes_bytes));
    if (!img)
        return fail(GCN10_E_INVAL, "%s: out of host memory", who);
    uint8_t *const planes = img + kLut16Bytes;
    ctx->weights_set = false;
    hipError_t e = hipMemcpy(img, ctx->d_lut16, kLut16Bytes, hipMemcpyDeviceToHost);
    for (int j = 0; j < k && e == hipSuccess; j++) {
        const uint16_t *const wj = w + 256 * j;
        uint8_t *const lo = planes + (size_t)(2 * j) * kLut16Bytes, *const hi = lo + kLut16Bytes;
        for (int i = 0; i < kLut16Bytes; i++) {
            const uint32_t v = img[i] == GCN10_NODATA ? 0u : wj[img[i]];
            lo[i] = (uint8_t)(v & 0xffu);
            hi[i] = (uint8_t)(v >> 8);
        }
    }
    memcpy(planes + (size_t)(2 * k) * kLut16Bytes, w, k * table_bytes);
    if (e == hipSuccess && !ctx->d_wlut)        // once, for the most tables a context takes
        e = hipMalloc(reinterpret_cast<void **>(&ctx->d_wlut),
                      GCN10_GPU_MAX_WEIGHT_TABLES * (2 * kLut16Bytes + table_bytes));
    // synchronous, as the images of set_tables: once per run, read by every later weighted call on any stream
    if (e == hipSuccess)
        e = hipMemcpy(ctx->d_wlut, planes, planes_bytes, hipMemcpyHostToDevice);
    free(img);
    HIP_TRY(e);
    ctx->weights_rising = 0u;
    for (int j = 0; j < k; j++)
        if (never_decreases(w + 256 * j))
            ctx->weights_rising |= 1u << j;
    ctx->n_weights = k;
    ctx->weights_set = true;
    return GCN10_OK;
}

}  // namespace

extern "C" {

int gcn10_gpu_grid_sums(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                        const int32_t *cellx, const int32_t *celly, int ncx, int ncy, unsigned cond_mask,
                        unsigned table_mask, unsigned long long *acc, gcn10_stream_t stream)
{
    return launch_sums(ctx, "gcn10_gpu_grid_sums", kPlain, esa, W, rows, cj, cellx, celly, ncx, ncy, cond_mask,
                       table_mask, acc, stream);
}

int gcn10_gpu_grid_finish(gcn10_gpu_ctx *ctx, const unsigned long long *acc, int n_sel, size_t n_cells,
                          uint8_t *means, const uint32_t *shared_idx, uint32_t n_shared, unsigned long long *shared,
                          gcn10_stream_t stream)
{
    return launch_finish(ctx, "gcn10_gpu_grid_finish", kPlain, acc, n_sel, n_cells, means, nullptr, shared_idx,
                         n_shared, shared, stream);
}

int gcn10_gpu_set_weights(gcn10_gpu_ctx *ctx, const uint16_t *w)
{
    return fold_weights(ctx, "gcn10_gpu_set_weights", w, 1);
}

int gcn10_gpu_set_weight_tables(gcn10_gpu_ctx *ctx, const uint16_t *w, int k)
{
    return fold_weights(ctx, "gcn10_gpu_set_weight_tables", w, k);
}

int gcn10_gpu_grid_sums_storms(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                               const int32_t *cellx, const int32_t *celly, int ncx, int ncy, unsigned cond_mask,
                               unsigned table_mask, unsigned long long *acc, gcn10_stream_t stream)
{
    return launch_sums(ctx, "gcn10_gpu_grid_sums_storms", kStorms, esa, W, rows, cj, cellx, celly, ncx, ncy, cond_mask,
                       table_mask, acc, stream);
}

int gcn10_gpu_grid_finish_storms(gcn10_gpu_ctx *ctx, const unsigned long long *acc, int n_sel, size_t n_cells,
                                 uint8_t *means, uint8_t *cnq, const uint32_t *shared_idx, uint32_t n_shared,
                                 unsigned long long *shared, gcn10_stream_t stream)
{
    return launch_finish(ctx, "gcn10_gpu_grid_finish_storms", kStorms, acc, n_sel, n_cells, means, cnq, shared_idx,
                         n_shared, shared, stream);
}

int gcn10_gpu_grid_sums_weighted(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                                 const int32_t *cellx, const int32_t *celly, int ncx, int ncy, unsigned cond_mask,
                                 unsigned table_mask, unsigned long long *acc, gcn10_stream_t stream)
{
    return launch_sums(ctx, "gcn10_gpu_grid_sums_weighted", kWeighted, esa, W, rows, cj, cellx, celly, ncx, ncy, cond_mask,
                       table_mask, acc, stream);
}

int gcn10_gpu_grid_finish_weighted(gcn10_gpu_ctx *ctx, const unsigned long long *acc, int n_sel, size_t n_cells,
                                   uint8_t *means, uint8_t *cnq, const uint32_t *shared_idx, uint32_t n_shared,
                                   unsigned long long *shared, gcn10_stream_t stream)
{
    return launch_finish(ctx, "gcn10_gpu_grid_finish_weighted", kWeighted, acc, n_sel, n_cells, means, cnq, shared_idx,
                         n_shared, shared, stream);
}

}  // extern "C"
