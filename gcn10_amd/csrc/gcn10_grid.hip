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
// Weighted sums (gcn10_gpu_grid_sums_weighted, DESIGN.md "Runoff-weighted composites"): a third word per (raster,
// cell), the sum of w[v] over the same pixels for a table w of 256 16-bit weights.  w o table is a function of (soil
// plane, landcover, table) like the value itself, so gcn10_gpu_set_weights folds w into two more images of the
// all-tables layout, the low and the high bytes of w[cn], zero where the CN image holds 255; against such an image the
// same gather, masks and dot products give the sum of the low and of the high bytes, and sw = lo + 256 hi.  In a
// weight plane 255 is a number: a plane pass makes no 255 test and no count.  A workgroup keeps its shape and gets a
// role besides its condition -- the CN image (words 0 and 1, exactly the unweighted kernel's), the low plane (word 2)
// or the high plane (word 2, shifted by 8) --, and the up to six workgroups of an item are dealt to one XCD.
//
// Several tables (gcn10_gpu_set_weight_tables, gcn10_gpu_grid_sums_storms, DESIGN.md "Several storms"): k tables are 2 k
// planes behind each other and 2 + k words per (raster, cell), word 2 + j the sum of w_j[v].  grid_sums_storms_kernel
// has 1 + 2 k roles per condition -- the CN image, then (low, high) of table 0, 1, ... --, dealt as above; the word
// count and a plane role's target word are run-time values of sum_item there, uniform, and enter only the addresses of
// the flush's atomics.  A plane role stages one image, so the LDS of a workgroup is the same.  The finish pass keeps
// k x 101 weights in LDS and decides per table between bisection and the scan from 1.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "gcn10_gpu_internal.hpp"
#include "gcn10_soil_readers.hpp"

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
    const uint8_t *lut[3];      // the CN image; the low and the high plane of the weights (weighted sums only)
    const int32_t *cellx, *celly;
    uint32_t W, rows, ncx, ncy;
    uint32_t chunks, band_rows;
    uint32_t items;             // chunks x bands
    uint32_t sel;               // bit r: raster r is selected
    uint32_t n_conds, conds[2]; // the selected conditions
    unsigned long long *acc;    // [n_sel][ncy][ncx][2], or [3] with weights
};

// the LDS of a workgroup: 62.3 KiB
struct GridLds {
    __attribute__((aligned(16))) uint8_t lut[kLut16Bytes];
    uint32_t sum[9 * kMaxCells], n255[9 * kMaxCells], area[kMaxCells];
    uint32_t cell_lo, cell_hi;
};

typedef u32x4 u32x4_u __attribute__((aligned(1)));

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
// WORDS per (raster, cell).  PLANE = true: against the weight plane `image`, its sums shifted by `shift` into word 2.
// WORDS = 0: `words` per (raster, cell) and a plane's sums into word `plane_word`, both uniform run-time values that
// enter the addresses of the flush's atomics only.
template <bool PLANE, uint32_t WORDS>
__device__ __forceinline__ void sum_item(const GridParams &p, GridLds &lds, const uint32_t item, const uint32_t cond,
                                         const uint8_t *image, const uint32_t shift, const uint32_t words = WORDS,
                                         const uint32_t plane_word = 2u)
{
    const uint32_t n_words = WORDS ? WORDS : words, to_word = WORDS ? 2u : plane_word;
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
                // one lane per cell: the plane's sum of every raster, shifted, to word 2
                for (uint32_t lc = threadIdx.x; lc < n_cells; lc += kThreads) {
                    for (uint32_t t = 0; t < 9; t++) {
                        if (!(sel9 & (1u << t)))
                            continue;
                        const uint32_t q = __popc(p.sel & ((1u << (9u * cond + t)) - 1u));
                        const uint32_t sv = sum[t * kMaxCells + lc];
                        sum[t * kMaxCells + lc] = 0u;
                        if (sv)
                            atomicAdd(p.acc + ((((size_t)q * p.ncy + cur) * p.ncx + c_lo + lc) * n_words + to_word),
                                      (unsigned long long)sv << shift);
                    }
                }
            }
            else {
                // lanes 2i and 2i + 1 add s and n of cell i: a wave's adds are 512 contiguous bytes (with weights: two
                // words of every three)
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
                            atomicAdd(p.acc + ((((size_t)q * p.ncy + cur) * p.ncx + c_lo + lc) * n_words + word),
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

// With R roles per item -- the conditions, times three with weights -- workgroups j, j + 8, ..., j + 8 (R - 1) of
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

__global__ __launch_bounds__(kThreads) void grid_sums_kernel(const GridParams p)
{
    __shared__ GridLds lds;
    uint32_t item, which;
    if (!deal_item(p, p.n_conds, item, which))
        return;
    sum_item<false, 2u>(p, lds, item, p.conds[which], p.lut[0], 0u);
}

// roles of an item: (condition, image), the three images of a condition next to each other
__global__ __launch_bounds__(kThreads) void grid_sums_weighted_kernel(const GridParams p)
{
    __shared__ GridLds lds;
    uint32_t item, role;
    if (!deal_item(p, 3u * p.n_conds, item, role))
        return;
    const uint32_t cond = p.conds[role / 3u], image = role % 3u;
    if (image == 0u)
        sum_item<false, 3u>(p, lds, item, cond, p.lut[0], 0u);
    else
        sum_item<true, 3u>(p, lds, item, cond, p.lut[image], image == 2u ? 8u : 0u);
}

// k tables: roles of an item (condition, image), the 1 + 2 k images of a condition next to each other -- the CN image,
// then (low, high) of table 0, 1, ...
struct StormParams {
    GridParams g;               // lut[1], lut[2]: not used
    const uint8_t *planes;      // [2 k] images: the low and the high plane of table 0, of table 1, ...
    uint32_t k;
};

__global__ __launch_bounds__(kThreads) void grid_sums_storms_kernel(const StormParams sp)
{
    __shared__ GridLds lds;
    const GridParams &p = sp.g;
    const uint32_t per = 1u + 2u * sp.k, words = 2u + sp.k;
    uint32_t item, role;
    if (!deal_item(p, per * p.n_conds, item, role))
        return;
    const uint32_t cond = p.conds[role / per], image = role % per;
    if (image == 0u)
        sum_item<false, 0u>(p, lds, item, cond, p.lut[0], 0u, words, 0u);
    else
        sum_item<true, 0u>(p, lds, item, cond, sp.planes + (size_t)(image - 1u) * kLut16Bytes,
                           (image & 1u) ? 0u : 8u, words, 2u + ((image - 1u) >> 1));
}

struct FinishParams {
    const unsigned long long *acc;
    size_t n_cells, total;      // cells per raster, and over all rasters
    uint8_t *means, *cnq;
    const uint32_t *shared_idx;
    uint32_t n_shared, n_sel;
    unsigned long long *shared;
    const uint16_t *weights;    // the context's, on the device (weighted finish only)
    uint32_t rising;            // weights[1..100] never decrease: bisection finds the smallest c
};

// the rule of gcn10_runoff_cn (include/gcn10_host.h), with w[0..100] in LDS
template <bool RISING>
__device__ __forceinline__ uint8_t runoff_cn(const uint32_t *w, unsigned long long s, unsigned long long n,
                                             unsigned long long sw)
{
    if (n == 0)
        return (uint8_t)GCN10_NODATA;
    if (sw == 0)
        return (uint8_t)((2ull * s + n) / (2ull * n));
    uint32_t lo = 1u, hi = 100u;
    if (RISING) {
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (n * w[mid] >= sw)
                hi = mid;
            else
                lo = mid + 1u;
        }
    }
    else {
        while (lo < hi && n * w[lo] < sw)
            lo++;
    }
    return (uint8_t)lo;
}

// WORDS = 2: the means and the shared pairs.  WORDS = 3: the means, the runoff-equivalent bytes and the shared triples.
template <uint32_t WORDS>
__global__ __launch_bounds__(kThreads) void grid_finish_kernel(const FinishParams p)
{
    __shared__ uint32_t w[101];
    if (WORDS == 3u) {
        for (uint32_t i = threadIdx.x; i < 101u; i += kThreads)
            w[i] = p.weights[i];
        __syncthreads();
    }
    const size_t stride = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < p.total; i += stride) {
        const unsigned long long s = p.acc[WORDS * i], n = p.acc[WORDS * i + 1u];
        p.means[i] = n == 0 ? (uint8_t)GCN10_NODATA : (uint8_t)((2ull * s + n) / (2ull * n));
        if (WORDS == 3u) {
            const unsigned long long sw = p.acc[WORDS * i + 2u];
            p.cnq[i] = p.rising ? runoff_cn<true>(w, s, n, sw) : runoff_cn<false>(w, s, n, sw);
        }
    }
    const size_t packed = (size_t)p.n_sel * p.n_shared;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < packed; i += stride) {
        const size_t q = i / p.n_shared, k = i - q * p.n_shared;
        const size_t at = q * p.n_cells + p.shared_idx[k];
#pragma unroll
        for (uint32_t word = 0; word < WORDS; word++)
            p.shared[WORDS * i + word] = p.acc[WORDS * at + word];
    }
}

// 2 + k words, k runoff-equivalent bytes per cell ([k][n_sel][n_cells]) and the shared cells' 2 + k words
struct StormFinishParams {
    FinishParams f;             // weights: [k][256]; rising: bit j for table j
    uint32_t k;
};

__global__ __launch_bounds__(kThreads) void grid_finish_storms_kernel(const StormFinishParams sp)
{
    __shared__ uint32_t w[GCN10_GPU_MAX_WEIGHT_TABLES * 101];
    const FinishParams &p = sp.f;
    const uint32_t k = sp.k, words = 2u + k;
    for (uint32_t i = threadIdx.x; i < k * 101u; i += kThreads)
        w[i] = p.weights[(i / 101u) * 256u + i % 101u];
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < p.total; i += stride) {
        const unsigned long long s = p.acc[words * i], n = p.acc[words * i + 1u];
        p.means[i] = n == 0 ? (uint8_t)GCN10_NODATA : (uint8_t)((2ull * s + n) / (2ull * n));
        for (uint32_t j = 0; j < k; j++) {
            const unsigned long long sw = p.acc[words * i + 2u + j];
            p.cnq[(size_t)j * p.total + i] = (p.rising >> j) & 1u ? runoff_cn<true>(w + 101u * j, s, n, sw)
                                                                  : runoff_cn<false>(w + 101u * j, s, n, sw);
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

enum SumsKind { kPlain, kWeighted, kStorms };      // pairs; triples of one table; 2 + k words of k tables

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
    if (!esa || !cj || !cellx || !celly || !acc || W <= 0 || rows <= 0 || ncx <= 0 || ncy <= 0)
        return fail(GCN10_E_INVAL, "%s: bad arguments W=%d rows=%d cells %d x %d (all > 0, no null pointer)", who, W,
                    rows, ncx, ncy);
    if ((rc = check_masks(ctx, who, cond_mask, table_mask)) != GCN10_OK)
        return rc;
    p.esa = esa;
    p.lut[0] = ctx->d_lut16;
    p.lut[1] = kind == kWeighted ? ctx->d_wlut : nullptr;
    p.lut[2] = kind == kWeighted ? ctx->d_wlut + kLut16Bytes : nullptr;
    p.cellx = cellx;
    p.celly = celly;
    p.W = (uint32_t)W;
    p.rows = (uint32_t)rows;
    p.ncx = (uint32_t)ncx;
    p.ncy = (uint32_t)ncy;
    p.acc = acc;
    uint32_t n_conds = 0;
    for (uint32_t r = 0; r < GCN10_N_RASTERS; r++)
        if (selected(r, cond_mask, table_mask))
            p.sel |= 1u << r;
    for (uint32_t cnd = 0; cnd < 2; cnd++)
        if ((p.sel >> (9u * cnd)) & 0x1ffu)
            p.conds[n_conds++] = cnd;
    const uint32_t k = kind == kStorms ? (uint32_t)ctx->n_weights : 1u;
    const uint32_t roles = kind == kPlain ? n_conds : (1u + 2u * k) * n_conds;
    p.chunks = (p.W + kChunkPx - 1u) / kChunkPx;
    // bands of at most kMaxBandRows rows, and shorter ones when the strip would not fill the device with them
    const uint32_t want = grid_cap(ctx, 8) / (p.chunks * roles) + 1u;
    p.band_rows = min(max((p.rows + want - 1u) / want, 16u), kMaxBandRows);
    const uint64_t items = (uint64_t)((p.rows + p.band_rows - 1u) / p.band_rows) * p.chunks;
    const uint64_t grid = roles > 1u ? (items + 7u) / 8u * (8u * roles) : items;
    if (grid > 0x7fffffffull)
        return fail(GCN10_E_INVAL, "%s: %llu workgroups; cut the strip into bands", who, (unsigned long long)grid);
    p.items = (uint32_t)items;
    p.n_conds = n_conds;
    if (kind == kStorms) {
        StormParams sp = {};
        sp.g = p;
        sp.planes = ctx->d_wlut;
        sp.k = k;
        hipLaunchKernelGGL(grid_sums_storms_kernel, dim3((uint32_t)grid), dim3(kThreads), 0, s, sp);
    }
    else if (kind == kWeighted)
        hipLaunchKernelGGL(grid_sums_weighted_kernel, dim3((uint32_t)grid), dim3(kThreads), 0, s, p);
    else
        hipLaunchKernelGGL(grid_sums_kernel, dim3((uint32_t)grid), dim3(kThreads), 0, s, p);
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
    const bool weighted = kind != kPlain;
    if ((rc = check_weights(ctx, who, kind)) != GCN10_OK)
        return rc;
    if (!acc || !means || (weighted && !cnq) || n_sel <= 0 || n_sel > GCN10_N_RASTERS || n_cells == 0 ||
        n_cells > 0xffffffffull || (n_shared && (!shared_idx || !shared)))
        return fail(GCN10_E_INVAL, "%s: bad arguments n_sel=%d n_cells=%zu n_shared=%u (1..%d rasters, 1..2^32-1 "
                    "cells, no null pointer)", who, n_sel, n_cells, n_shared, GCN10_N_RASTERS);
    FinishParams p = {};
    p.acc = acc;
    p.n_cells = n_cells;
    p.total = n_cells * (size_t)n_sel;
    p.means = means;
    p.cnq = cnq;
    p.shared_idx = shared_idx;
    p.n_shared = n_shared;
    p.n_sel = (uint32_t)n_sel;
    p.shared = shared;
    p.weights = weighted ? reinterpret_cast<const uint16_t *>(ctx->d_wlut + 2 * ctx->n_weights * kLut16Bytes) : nullptr;
    p.rising = ctx->weights_rising;
    const uint32_t grid = stream_grid(ctx, (p.total + kThreads - 1u) / kThreads);
    if (kind == kStorms) {
        StormFinishParams sp = {};
        sp.f = p;
        sp.k = (uint32_t)ctx->n_weights;
        hipLaunchKernelGGL(grid_finish_storms_kernel, dim3(grid), dim3(kThreads), 0, s, sp);
    }
    else if (weighted)
        hipLaunchKernelGGL(grid_finish_kernel<3u>, dim3(grid), dim3(kThreads), 0, s, p);
    else
        hipLaunchKernelGGL(grid_finish_kernel<2u>, dim3(grid), dim3(kThreads), 0, s, p);
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
    for (int j = 0; j < k; j++) {
        bool rising = true;
        for (int c = 2; c <= 100; c++)
            if (w[256 * j + c] < w[256 * j + c - 1])
                rising = false;
        if (rising)
            ctx->weights_rising |= 1u << j;
    }
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
