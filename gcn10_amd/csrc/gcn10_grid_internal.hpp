// gcn10_grid_internal.hpp -- what the model-grid files of libgcn10_gpu.so share, each piece once:
//   gcn10_grid.hip        sums with one weight table per launch, folded into image planes (0 to 8 tables)
//   gcn10_grid_rain.hip   sums with the weight table chosen per cell, from the cells' pair histograms
//   gcn10_grid_rains.hip  the same with 1 to 8 tables per cell, the histograms counted once
//                         (the counting itself: gcn10_grid_rain_piece.hpp)
// The device side is the two byte rules of a cell; the host side is what their sums and finish calls check and size
// alike.
#ifndef GCN10_GRID_INTERNAL_HPP
#define GCN10_GRID_INTERNAL_HPP

#include "gcn10_gpu_internal.hpp"
#include "gcn10_soil_readers.hpp"

namespace gcn10 {

typedef u32x4 u32x4_u __attribute__((aligned(1)));

// the byte of the mean of n values that add up to s, as the area means round it
__device__ __forceinline__ uint8_t mean_byte(unsigned long long s, unsigned long long n)
{
    return n == 0 ? (uint8_t)GCN10_NODATA : (uint8_t)((2ull * s + n) / (2ull * n));
}

// the rule of gcn10_runoff_cn (include/gcn10_host.h) against the weights w[0..100]: 32-bit words in LDS or the 16-bit
// table in global memory.  rising: w[1..100] never decreases, so bisection finds the smallest c
template <typename T>
__device__ __forceinline__ uint8_t runoff_cn(const T *w, bool rising, unsigned long long s, unsigned long long n,
                                             unsigned long long sw)
{
    if (n == 0)
        return (uint8_t)GCN10_NODATA;
    if (sw == 0)
        return mean_byte(s, n);
    uint32_t lo = 1u, hi = 100u;
    if (rising) {
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

// w[1..100] never decreases
inline bool never_decreases(const uint16_t *w)
{
    for (int c = 2; c <= 100; c++)
        if (w[c] < w[c - 1])
            return false;
    return true;
}

// bit r of the result: raster r is selected; conds[0 .. n_conds): the conditions with a selected raster
inline uint32_t select_rasters(unsigned cond_mask, unsigned table_mask, uint32_t (&conds)[2], uint32_t &n_conds)
{
    uint32_t sel = 0u;
    for (uint32_t r = 0; r < GCN10_N_RASTERS; r++)
        if (selected(r, cond_mask, table_mask))
            sel |= 1u << r;
    n_conds = 0u;
    for (uint32_t cnd = 0; cnd < 2; cnd++)
        if ((sel >> (9u * cnd)) & 0x1ffu)
            conds[n_conds++] = cnd;
    return sel;
}

// the arguments of a sums call; extra: the pointers that only this call takes are there
inline int check_sums_args(const char *who, const uint8_t *esa, int W, int rows, const int32_t *cj,
                           const int32_t *cellx, const int32_t *celly, int ncx, int ncy,
                           const unsigned long long *acc, bool extra = true)
{
    if (!esa || !cj || !cellx || !celly || !extra || !acc || W <= 0 || rows <= 0 || ncx <= 0 || ncy <= 0)
        return fail(GCN10_E_INVAL, "%s: bad arguments W=%d rows=%d cells %d x %d (all > 0, no null pointer)", who, W,
                    rows, ncx, ncy);
    return GCN10_OK;
}

// the arguments of a finish call; extra: the pointers that only this call takes, or needs, are there
inline int check_finish_args(const char *who, const unsigned long long *acc, int n_sel, size_t n_cells,
                             const uint8_t *means, const uint32_t *shared_idx, uint32_t n_shared,
                             const unsigned long long *shared, bool extra = true)
{
    if (!acc || !means || !extra || n_sel <= 0 || n_sel > GCN10_N_RASTERS || n_cells == 0 ||
        n_cells > 0xffffffffull || (n_shared && (!shared_idx || !shared)))
        return fail(GCN10_E_INVAL, "%s: bad arguments n_sel=%d n_cells=%zu n_shared=%u (1..%d rasters, 1..2^32-1 "
                    "cells, no null pointer)", who, n_sel, n_cells, n_shared, GCN10_N_RASTERS);
    return GCN10_OK;
}

// GCN10_E_STATE unless gcn10_gpu_set_rain_tables has run (gcn10_grid_rain.hip, gcn10_grid_rains.hip, gcn10_zonal_rain.hip)
inline int check_rain_tables(gcn10_gpu_ctx *ctx, const char *who)
{
    if (ctx->n_rain_tables < 1)
        return fail(GCN10_E_STATE, "%s: call gcn10_gpu_set_rain_tables first", who);
    return GCN10_OK;
}

// Rows of a band: at most `cap`, and fewer (`floor` at least) when the strip would not fill the device -- per_cu
// workgroups on every compute unit -- with bands that tall; n: the workgroups of one band
inline uint32_t band_height(const gcn10_gpu_ctx *ctx, int per_cu, uint32_t n, uint32_t rows, uint32_t floor,
                            uint32_t cap)
{
    const uint32_t want = grid_cap(ctx, per_cu) / n + 1u;
    return min(max((rows + want - 1u) / want, floor), cap);
}

}  // namespace gcn10

#endif
