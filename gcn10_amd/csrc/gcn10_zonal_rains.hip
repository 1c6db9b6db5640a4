// gcn10_zonal_rains.hip -- the words {s, n, sw_1 .. sw_k} of every selected raster over the pixels of zones, with a TUPLE
// of k weight tables chosen per item (config key zone_rains=..., DESIGN.md "Several rainfall rasters under zones").
//
// The host cuts the spans of a zone wherever the byte of ANY of its k rainfall rasters changes (gcn10_zone_rains_cut) and
// hands over spans sorted by (zone, tuple) and items {first_span, n_spans, table[8]}.  The workgroup, the walk over the
// items and the listing of the non-zero bins are those of zonal_sums_rain_kernel (gcn10_zonal_rain_walk.hpp): the pixels
// of a (zone, tuple) are counted ONCE into the 16 KiB LDS pair histogram, whatever k is.  The flush deals one (bin,
// condition) to a thread, which reads the nine values of its bin once and then, layer after layer, the nine weights from
// tables + 256 * table[j]: c * v and c go to words 0 and 1, c * w_j[v] to word 2 + j of 18 * (2 + k) 64-bit LDS words;
// one 64-bit global atomic per non-zero (raster, word) follows.  One kernel serves k = 1..8; the layer loop runs on a
// workgroup-uniform count.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gcn10_grid_internal.hpp"
#include "gcn10_pair_hist.hpp"
#include "gcn10_zonal_rain_walk.hpp"

using namespace gcn10;
using namespace gcn10::pair_hist;
using namespace gcn10::zonal_rain_walk;

namespace {

constexpr uint32_t kMaxLayers = GCN10_GPU_MAX_RAIN_LAYERS;
constexpr uint32_t kMaxSums = 2u * 9u * (2u + kMaxLayers);     // (condition, table, word)
static_assert(kMaxSums <= (uint32_t)kThreads, "one thread per sum at the end of a flush");
static_assert(sizeof(gcn10_zone_rains_item) == 16 && kMaxLayers == 8, "a tuple is the 8 bytes behind two words");

struct ZonalRainsParams {
    const uint8_t *esa;             // strip, W x rows, row major
    SoilView soil;                  // soil code bytes, soil row of every strip row
    const uint8_t *lut;             // the all-tables image, in global memory
    const gcn10_zone_span *spans;
    const gcn10_zone_rains_item *items;
    const uint16_t *tables;         // [n_tables][256]
    uint32_t n_tables;
    uint32_t W, n_items, items_per_wg;
    uint32_t k;                     // layers, 1..8
    uint64_t tuple_mask;            // bytes 0..k-1 of a tuple
    uint32_t sel;                   // bit r: raster r is selected
    uint32_t n_sel;
    uint32_t n_conds, conds[2];     // the selected conditions
    unsigned long long *acc;        // [n_zones][n_sel][2 + k]
};

// The workgroup's histogram against the tables of `tuple` (layer j in bits 8 j .. 8 j + 7), added to the words of `zone`;
// h is all zero afterwards.
__device__ __forceinline__ void flush_piece(const ZonalRainsParams &p, uint32_t *h, unsigned long long *sums,
                                            uint16_t *list, uint32_t *n_list, uint32_t zone, uint64_t tuple)
{
    const uint32_t tid = threadIdx.x, words = 2u + p.k, n_sums = 18u * words;
    if (tid < n_sums)
        sums[tid] = 0ull;
    if (tid == 0)
        *n_list = 0u;
    __syncthreads();            // the counts of every lane are in h, the sums and the list are empty
    list_bins(h, list, n_list);
    __syncthreads();
    const uint32_t m = *n_list, two = p.n_conds == 2u ? 1u : 0u;
    for (uint32_t u = tid; u < (m << two); u += kThreads) {
        const uint32_t i = list[u >> two], c = h[i];
        const uint32_t cond = p.conds[u & two], sel9 = (p.sel >> (9u * cond)) & 0x1ffu;
        unsigned long long *const to = sums + cond * 9u * words;
        uint32_t v[9];
        bin_values(p.lut, i, cond, v);
#pragma unroll
        for (uint32_t t = 0; t < 9; t++)
            if ((sel9 >> t) & 1u && v[t] != GCN10_NODATA) {
                atomicAdd(to + t * words + 0, (unsigned long long)c * v[t]);
                atomicAdd(to + t * words + 1, (unsigned long long)c);
            }
        for (uint32_t j = 0; j < p.k; j++) {
            const uint32_t table = (uint32_t)(tuple >> (8u * j)) & 255u;
            const uint16_t *const w = p.tables + 256u * (table < p.n_tables ? table : 0u);
            uint32_t wv[9];
#pragma unroll
            for (uint32_t t = 0; t < 9; t++)
                wv[t] = w[v[t]];        // w[255] is there and never used
#pragma unroll
            for (uint32_t t = 0; t < 9; t++)
                if ((sel9 >> t) & 1u && v[t] != GCN10_NODATA)
                    atomicAdd(to + t * words + 2u + j, (unsigned long long)c * wv[t]);
        }
    }
    __syncthreads();
    for (uint32_t j = tid; j < m; j += kThreads)
        h[list[j]] = 0u;
    if (tid < n_sums) {
        const unsigned long long total = sums[tid];
        const uint32_t r = tid / words, word = tid - words * r;     // sums of a raster that is not selected are zero
        if (total) {
            const uint32_t q = __popc(p.sel & ((1u << r) - 1u));
            atomicAdd(p.acc + ((size_t)zone * p.n_sel + q) * words + word, total);
        }
    }
    __syncthreads();            // sums, the list and h may be written again
}

__global__ __launch_bounds__(kThreads) void zonal_sums_rains_kernel(const ZonalRainsParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t h[kHistWords];
    __shared__ unsigned long long sums[kMaxSums];
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
    uint64_t cur_tuple = 0ull;
    for (uint32_t it = first; it < last; it++) {            // workgroup uniform throughout
        const gcn10_zone_rains_item item = p.items[it];
        const uint32_t first_span = item.first_span, n_spans = item.n_spans;
        uint64_t tuple;
        __builtin_memcpy(&tuple, item.table, sizeof tuple);
        tuple &= p.tuple_mask;      // bytes k..7 pick no table
        if (n_spans == 0u)
            continue;
        const int32_t zone = p.spans[first_span].zone;
        if (zone != cur_zone || tuple != cur_tuple) {
            if (cur_zone >= 0)
                flush_piece(p, h, sums, list, &n_list, (uint32_t)cur_zone, cur_tuple);
            cur_zone = zone;
            cur_tuple = tuple;
        }
        count_item(p.esa, p.soil, p.W, p.spans, first_span, n_spans, h, walk);
    }
    if (cur_zone >= 0)
        flush_piece(p, h, sums, list, &n_list, (uint32_t)cur_zone, cur_tuple);
}

}  // namespace

extern "C" {

int gcn10_gpu_zonal_sums_rains(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                               const gcn10_zone_span *spans_dev, const gcn10_zone_rains_item *items_dev, size_t n_items,
                               int n_zones, unsigned cond_mask, unsigned table_mask, int k, unsigned long long *acc,
                               gcn10_stream_t stream)
{
    const char *const who = "gcn10_gpu_zonal_sums_rains";
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (k < 1 || k > (int)kMaxLayers)
        return fail(GCN10_E_INVAL, "%s: k=%d outside 1..%u", who, k, kMaxLayers);
    if (n_items == 0)
        return GCN10_OK;
    hipStream_t s = as_stream(ctx, stream);
    ZonalRainsParams p = {};
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
    p.k = (uint32_t)k;
    p.tuple_mask = k == 8 ? ~0ull : (1ull << (8 * k)) - 1ull;
    p.sel = select_rasters(cond_mask, table_mask, p.conds, p.n_conds);
    p.n_sel = (uint32_t)__builtin_popcount(p.sel);
    const uint64_t cap = grid_cap(ctx, kGridPerCu);
    const uint32_t grid = (uint32_t)(n_items < cap ? n_items : cap);
    p.items_per_wg = (p.n_items + grid - 1u) / grid;
    hipLaunchKernelGGL(zonal_sums_rains_kernel, dim3(grid), dim3(kThreads), 0, s, p);
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}

}  // extern "C"
