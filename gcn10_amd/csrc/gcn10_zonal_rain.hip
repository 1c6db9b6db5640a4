// gcn10_zonal_rain.hip -- the triples {s, n, sw} of every selected raster over the pixels of zones, with the weight
// table chosen PER ITEM (config key zone_rain=..., DESIGN.md "Rainfall raster under zones").
//
// The host cuts the spans of a zone where the rainfall byte changes (gcn10_zone_rain_cut) and hands over spans sorted
// by (zone, byte) and items {first_span, n_spans, table}: runs of consecutive spans of ONE zone under ONE table.  The
// workgroup, the span staging and the dealing of 16-pixel groups to the lanes are those of zonal_pair_histogram_kernel
// (gcn10_zonal.hip); a workgroup takes a contiguous run of items and keeps the 16 KiB LDS pair histogram of the
// (zone, table) at hand.  What differs is the flush, when either changes and at the end: not "copy 4096 bins to the
// zone" but "apply the table of this piece of the zone and add 18 triples" -- every raster's value at a pixel is a
// function of the pixel's pair (gcn10_stats.hip), so a non-zero bin (count c) gives c * v, c and c * w[v] for each
// selected raster, v from the all-tables image in global memory (lut16_row) and w = tables + 256 * table.  The 54
// (condition, table, word) sums are 64-bit words in LDS (a run may count up to 2^32 pixels, and c * w[v] passes 2^32 at
// 65 537 pixels), then ONE 64-bit global atomic per non-zero (raster, word), and the histogram is zero again.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gcn10_grid_internal.hpp"
#include "gcn10_pair_hist.hpp"
#include "gcn10_zonal_rain_walk.hpp"

using namespace gcn10;
using namespace gcn10::pair_hist;
using namespace gcn10::zonal_rain_walk;

namespace {

constexpr uint32_t kSums = 2u * 9u * 3u;                    // (condition, table, word)

struct ZonalRainParams {
    const uint8_t *esa;             // strip, W x rows, row major
    SoilView soil;                  // soil code bytes, soil row of every strip row
    const uint8_t *lut;             // the all-tables image, in global memory
    const gcn10_zone_span *spans;
    const gcn10_zone_rain_item *items;
    const uint16_t *tables;         // [n_tables][256]
    uint32_t n_tables;
    uint32_t W, n_items, items_per_wg;
    uint32_t sel;                   // bit r: raster r is selected
    uint32_t n_sel;
    uint32_t n_conds, conds[2];     // the selected conditions
    unsigned long long *acc;        // [n_zones][n_sel][3]
};

// The workgroup's histogram against table `table`, added to the triples of `zone`; h is all zero afterwards.  The non-zero
// bins are listed and dealt one (bin, condition) to a thread (list_bins says why).
__device__ __forceinline__ void flush_piece(const ZonalRainParams &p, uint32_t *h, unsigned long long *sums,
                                            uint16_t *list, uint32_t *n_list, uint32_t zone, uint32_t table)
{
    const uint32_t tid = threadIdx.x;
    if (tid < kSums)
        sums[tid] = 0ull;
    if (tid == 0)
        *n_list = 0u;
    __syncthreads();            // the counts of every lane are in h, the sums and the list are empty
    list_bins(h, list, n_list);
    __syncthreads();
    const uint32_t m = *n_list, two = p.n_conds == 2u ? 1u : 0u;
    const uint16_t *const w = p.tables + 256u * (table < p.n_tables ? table : 0u);
    for (uint32_t u = tid; u < (m << two); u += kThreads) {
        const uint32_t i = list[u >> two], c = h[i];
        const uint32_t cond = p.conds[u & two], sel9 = (p.sel >> (9u * cond)) & 0x1ffu;
        uint32_t v[9], wv[9];
        bin_values(p.lut, i, cond, v);
#pragma unroll
        for (uint32_t t = 0; t < 9; t++)
            wv[t] = w[v[t]];            // w[255] is there and never used
#pragma unroll
        for (uint32_t t = 0; t < 9; t++)
            if ((sel9 >> t) & 1u && v[t] != GCN10_NODATA) {
                unsigned long long *const to = sums + (cond * 9u + t) * 3u;
                atomicAdd(to + 0, (unsigned long long)c * v[t]);
                atomicAdd(to + 1, (unsigned long long)c);
                atomicAdd(to + 2, (unsigned long long)c * wv[t]);
            }
    }
    __syncthreads();
    for (uint32_t j = tid; j < m; j += kThreads)
        h[list[j]] = 0u;
    if (tid < kSums) {
        const unsigned long long total = sums[tid];
        const uint32_t r = tid / 3u, word = tid - 3u * r;   // sums of a raster that is not selected are zero
        if (total) {
            const uint32_t q = __popc(p.sel & ((1u << r) - 1u));
            atomicAdd(p.acc + ((size_t)zone * p.n_sel + q) * 3u + word, total);
        }
    }
    __syncthreads();            // sums, the list and h may be written again
}

__global__ __launch_bounds__(kThreads) void zonal_sums_rain_kernel(const ZonalRainParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t h[kHistWords];
    __shared__ unsigned long long sums[kSums];
    __shared__ uint16_t list[kHistWords];           // the non-zero bins of a flush
    __shared__ uint32_t n_list;
    __shared__ WalkLds walk;

    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < (uint32_t)kHistWords; i += kThreads)
        h[i] = 0u;
    __syncthreads();

    const uint32_t first = blockIdx.x * p.items_per_wg;
    const uint32_t last = min(first + p.items_per_wg, p.n_items);
    int32_t cur_zone = -1;
    uint32_t cur_table = 0u;
    for (uint32_t it = first; it < last; it++) {            // workgroup uniform throughout
        const gcn10_zone_rain_item item = p.items[it];
        const uint32_t first_span = item.first_span, n_spans = item.n_spans;
        if (n_spans == 0u)
            continue;
        const int32_t zone = p.spans[first_span].zone;
        if (zone != cur_zone || item.table != cur_table) {
            if (cur_zone >= 0)
                flush_piece(p, h, sums, list, &n_list, (uint32_t)cur_zone, cur_table);
            cur_zone = zone;
            cur_table = item.table;
        }
        count_item(p.esa, p.soil, p.W, p.spans, first_span, n_spans, h, walk);
    }
    if (cur_zone >= 0)
        flush_piece(p, h, sums, list, &n_list, (uint32_t)cur_zone, cur_table);
}

}  // namespace

extern "C" {

int gcn10_gpu_zonal_sums_rain(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                              const gcn10_zone_span *spans_dev, const gcn10_zone_rain_item *items_dev, size_t n_items,
                              int n_zones, unsigned cond_mask, unsigned table_mask, unsigned long long *acc,
                              gcn10_stream_t stream)
{
    const char *const who = "gcn10_gpu_zonal_sums_rain";
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (n_items == 0)
        return GCN10_OK;
    hipStream_t s = as_stream(ctx, stream);
    ZonalRainParams p = {};
    if ((rc = check_tables(ctx, who)) != GCN10_OK)
        return rc;
    if ((rc = check_rain_tables(ctx, who)) != GCN10_OK)
        return rc;
    if ((rc = bind_soil(ctx, who, W, s, cj, &p.soil)) != GCN10_OK)
        return rc;
    if (!esa || !cj || !spans_dev || !items_dev || !acc || W <= 0 || rows <= 0 || n_zones <= 0 || n_items > 0xffffffffu)
        return fail(GCN10_E_INVAL, "%s: bad arguments W=%d rows=%d zones=%d items=%zu", who, W, rows, n_zones, n_items);
    if ((rc = check_masks(ctx, who, cond_mask, table_mask)) != GCN10_OK)
        return rc;
    p.esa = esa;
    p.lut = ctx->d_lut16;
    p.spans = spans_dev;
    p.items = items_dev;
    p.tables = ctx->d_rain_tables;
    p.n_tables = (uint32_t)ctx->n_rain_tables;
    p.acc = acc;
    p.W = (uint32_t)W;
    p.n_items = (uint32_t)n_items;
    p.sel = select_rasters(cond_mask, table_mask, p.conds, p.n_conds);
    p.n_sel = (uint32_t)__builtin_popcount(p.sel);
    const uint64_t cap = grid_cap(ctx, kGridPerCu);
    const uint32_t grid = (uint32_t)(n_items < cap ? n_items : cap);
    p.items_per_wg = (p.n_items + grid - 1u) / grid;
    hipLaunchKernelGGL(zonal_sums_rain_kernel, dim3(grid), dim3(kThreads), 0, s, p);
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}

}  // extern "C"
