// gcn10_overview.hip -- overview levels of the Cloud Optimized GeoTIFF output (config key cog=1).
//
// Level k of a W x H block is ceil(W / 2^k) x ceil(H / 2^k) pixels.  Two resamplings ("Cloud
// Optimized GeoTIFF output"):
//
//   nearest  level k pixel (x, y) = full-resolution pixel (min(2^k x + 2^(k-1), W-1), min(2^k y + 2^(k-1), H-1)).
//            Such a level is a block in its own right: gcn10_gpu_overview_nearest gathers its landcover from the
//            block's landcover, the host composes the soil index maps the same way, and the run's own encoders
//            (fused, per raster, LZW) take it from there.
//   average  level k pixel = the clipped 2x2 footprint in level k-1 (level 0 = full resolution) with the value
//            255 left out: (2 s + n) / (2 n), rounded half up, 255 when n = 0.  gcn10_gpu_overview_average
//            computes level 1 straight from landcover + prepared soil + byte tables (no full-resolution CN
//            raster), then levels 2.. from level 1 inside one workgroup per 256 x 256 full-resolution tile.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gcn10_gpu_internal.hpp"
#include "gcn10_soil_readers.hpp"

using namespace gcn10;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxLevels = 8;               // a 256 x 256 full-resolution tile holds whole pixels of levels 1..8
constexpr int kL1Tile = 128;                // level-1 pixels per workgroup side (= 256 full-resolution pixels)
// level-1 rows per workgroup of the level-1 kernel; per 36000² block: 1 row 9.5 ms, 4 rows 9.2, 32 rows 10.5
// (COG output)
constexpr uint32_t kL1Rows = 4;

__device__ __forceinline__ uint8_t avg_of(uint32_t s, uint32_t n)
{
    return n == 0 ? (uint8_t)GCN10_NODATA : (uint8_t)((2u * s + n) / (2u * n));
}

struct NearestParams {
    const uint8_t *src;
    uint8_t *dst;
    uint32_t W, H, Wk, Hk, level;
};

__global__ __launch_bounds__(kThreads) void overview_nearest_kernel(const NearestParams p)
{
    const uint32_t x = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t y = blockIdx.y;
    if (x >= p.Wk || y >= p.Hk)
        return;
    const uint32_t half = 1u << (p.level - 1u);
    const uint32_t sx = min((x << p.level) + half, p.W - 1u);
    const uint32_t sy = min((y << p.level) + half, p.H - 1u);
    p.dst[(size_t)y * p.Wk + x] = p.src[(size_t)sy * p.W + sx];
}

// ---- average, level 1 ----------------------------------------------------
// One thread per level-1 pixel: its (up to) four full-resolution pixels are read once, and every selected raster's
// value of each comes from ONE 16-byte LDS read per pixel and condition (the nine tables' bytes of a (soil plane,
// landcover) pair lie side by side, as the strip kernels read them).  A wave's 64 reads of a row hit 16 distinct
// bank groups at most (the rows are 16 bytes = 4 banks apart), and lanes that share a landcover value share the
// address (a broadcast); per-raster byte look-ups, one per raster and pixel, would cost 18x the LDS instructions.
struct AvgParams {
    const uint8_t *esa;         // block row 0
    SoilView soil;              // prepared soil codes, block's soil row of every row
    const uint8_t *lut16;
    uint32_t W, H, y1_begin, y1_end;        // level-1 rows of this strip
    uint32_t cond_mask, table_mask;
    uint32_t n_levels;
    uint8_t *out[GCN10_N_RASTERS][kMaxLevels];  // [raster][k - 1]; NULL for a raster not selected
};

__device__ __forceinline__ void level1_pixel(const AvgParams &p, const uint8_t *lut, uint32_t W1, uint32_t x1,
                                             uint32_t y1);

// A workgroup takes 256 level-1 columns of kL1Rows rows, so the 24.6 KB table image is staged into LDS once per
// kL1Rows rows.  With one row per workgroup the staging re-reads 31 GB from L2 per 36000² block, but cutting that
// 32-fold does not speed the kernel up (its time is latency: one level-1 pixel per lane and row).
__global__ __launch_bounds__(kThreads) void overview_avg_level1_kernel(const AvgParams p)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[kLut16Bytes];
    stage_lut16<kThreads>(lut, p.lut16);
    __syncthreads();

    const uint32_t W1 = (p.W + 1u) >> 1;
    const uint32_t x1 = blockIdx.x * kThreads + threadIdx.x;
    if (x1 >= W1)
        return;
    const uint32_t y1_end = min(p.y1_begin + (blockIdx.y + 1u) * kL1Rows, p.y1_end);
    for (uint32_t y1 = p.y1_begin + blockIdx.y * kL1Rows; y1 < y1_end; y1++)
        level1_pixel(p, lut, W1, x1, y1);
}

__device__ __forceinline__ void level1_pixel(const AvgParams &p, const uint8_t *lut, uint32_t W1, uint32_t x1,
                                             uint32_t y1)
{
    uint32_t s[GCN10_N_RASTERS], n[GCN10_N_RASTERS];
#pragma unroll
    for (int r = 0; r < GCN10_N_RASTERS; r++)
        s[r] = n[r] = 0;
    for (uint32_t dy = 0; dy < 2; dy++) {
        const uint32_t y = 2u * y1 + dy;
        if (y >= p.H)
            break;
        const uint32_t crow = p.soil.row(y);
        for (uint32_t dx = 0; dx < 2; dx++) {
            const uint32_t x = 2u * x1 + dx;
            if (x >= p.W)
                break;
            const uint32_t lc = p.esa[(size_t)y * p.W + x];
            const uint32_t cd = *p.soil.at(crow, x);
#pragma unroll
            for (int c = 0; c < 2; c++) {
                if (!(p.cond_mask & (1u << c)))
                    continue;
                const uint32_t plane = min((cd >> (4 * c)) & 0xfu, (uint32_t)kPlanes - 1u);
                const u32x4 row = *reinterpret_cast<const u32x4 *>(lut16_row(lut, plane, lc));
#pragma unroll
                for (int k = 0; k < 9; k++) {
                    const uint32_t v = (row[k >> 2] >> (8 * (k & 3))) & 0xffu;
                    const bool use = v != GCN10_NODATA;
                    s[c * 9 + k] += use ? v : 0u;
                    n[c * 9 + k] += use ? 1u : 0u;
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < GCN10_N_RASTERS; r++) {
        uint8_t *o = p.out[r][0];
        if (o && selected(r, p.cond_mask, p.table_mask))
            o[(size_t)y1 * W1 + x1] = avg_of(s[r], n[r]);
    }
}

// ---- average, levels 2 .. n_levels from level 1 --------------------------
// One workgroup per (raster, 256 x 256 full-resolution tile): the tile's 128 x 128 level-1 pixels go to LDS once,
// and every deeper level is reduced there (ping-pong between a 16 KB and a 4 KB buffer) and written out.  A tile's
// origin is a multiple of 2 at every level < 8, so no footprint crosses a tile edge.
__global__ __launch_bounds__(kThreads) void overview_avg_deeper_kernel(const AvgParams p, uint32_t ty0)
{
    __shared__ uint8_t a[kL1Tile * kL1Tile];
    __shared__ uint8_t b[(kL1Tile / 2) * (kL1Tile / 2)];
    const uint32_t r = blockIdx.z;
    if (!selected(r, p.cond_mask, p.table_mask) || !p.out[r][0])
        return;
    const uint32_t tx = blockIdx.x, ty = ty0 + blockIdx.y;
    uint32_t Wl = (p.W + 1u) >> 1, Hl = (p.H + 1u) >> 1;     // level-1 size
    uint32_t side = kL1Tile;
    uint32_t w = min(side, Wl - tx * side), h = min(side, Hl - ty * side);
    const uint8_t *l1 = p.out[r][0];
    for (uint32_t i = threadIdx.x; i < w * h; i += kThreads) {
        const uint32_t yy = i / w, xx = i - yy * w;
        a[yy * side + xx] = l1[(size_t)(ty * side + yy) * Wl + tx * side + xx];
    }
    __syncthreads();
    uint8_t *cur = a, *nxt = b;
    for (uint32_t k = 2; k <= p.n_levels; k++) {
        const uint32_t Wk = (Wl + 1u) >> 1, Hk = (Hl + 1u) >> 1;
        const uint32_t wk = (w + 1u) >> 1, hk = (h + 1u) >> 1, sidek = side >> 1;
        uint8_t *o = p.out[r][k - 1];
        for (uint32_t i = threadIdx.x; i < wk * hk; i += kThreads) {
            const uint32_t yy = i / wk, xx = i - yy * wk;
            uint32_t s = 0, n = 0;
#pragma unroll
            for (uint32_t dy = 0; dy < 2; dy++)
#pragma unroll
                for (uint32_t dx = 0; dx < 2; dx++) {
                    const uint32_t sx = 2u * xx + dx, sy = 2u * yy + dy;
                    if (sx < w && sy < h) {
                        const uint32_t v = cur[sy * side + sx];
                        s += v != GCN10_NODATA ? v : 0u;
                        n += v != GCN10_NODATA ? 1u : 0u;
                    }
                }
            const uint8_t v = avg_of(s, n);
            nxt[yy * sidek + xx] = v;
            o[(size_t)(ty * sidek + yy) * Wk + tx * sidek + xx] = v;
        }
        __syncthreads();
        uint8_t *t = cur;
        cur = nxt;
        nxt = t;
        Wl = Wk;
        Hl = Hk;
        w = wk;
        h = hk;
        side = sidek;
    }
}

}  // namespace

extern "C" {

int gcn10_gpu_overview_nearest(gcn10_gpu_ctx *ctx, const uint8_t *src, int W, int H, int level, uint8_t *dst,
                               gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (!src || !dst || W <= 0 || H <= 0 || level < 1 || level > 30)
        return fail(GCN10_E_INVAL, "gcn10_gpu_overview_nearest: bad arguments W=%d H=%d level=%d", W, H, level);
    NearestParams p;
    p.src = src;
    p.dst = dst;
    p.W = (uint32_t)W;
    p.H = (uint32_t)H;
    p.level = (uint32_t)level;
    p.Wk = (uint32_t)(((int64_t)W + (1ll << level) - 1) >> level);
    p.Hk = (uint32_t)(((int64_t)H + (1ll << level) - 1) >> level);
    dim3 grid((p.Wk + kThreads - 1) / kThreads, p.Hk);
    hipLaunchKernelGGL(overview_nearest_kernel, grid, dim3(kThreads), 0, as_stream(ctx, stream), p);
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}

int gcn10_gpu_overview_average(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int H, int y0, int rows,
                               const int32_t *cj, unsigned cond_mask, unsigned table_mask, int n_levels,
                               uint8_t *const *levels, gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    const char *const who = "gcn10_gpu_overview_average";
    hipStream_t s = as_stream(ctx, stream);
    AvgParams p = {};
    if ((rc = check_tables(ctx, who)) != GCN10_OK || (rc = bind_soil(ctx, who, W, s, cj, &p.soil)) != GCN10_OK)
        return rc;
    if (!esa || !cj || !levels || W <= 0 || H <= 0 || n_levels < 1 || n_levels > kMaxLevels || y0 < 0 ||
        rows <= 0 || y0 % 256 != 0 || y0 + rows > H || (rows % 256 != 0 && y0 + rows != H))
        return fail(GCN10_E_INVAL, "gcn10_gpu_overview_average: bad strip y0=%d rows=%d of %dx%d, %d levels "
                    "(strips start and end on multiples of 256 rows, 1..8 levels)", y0, rows, W, H, n_levels);
    if ((rc = check_masks(ctx, who, cond_mask, table_mask)) != GCN10_OK)
        return rc;
    p.esa = esa;
    p.lut16 = ctx->d_lut16;
    p.W = (uint32_t)W;
    p.H = (uint32_t)H;
    p.cond_mask = cond_mask;
    p.table_mask = table_mask;
    p.n_levels = (uint32_t)n_levels;
    int q = 0;
    for (int r = 0; r < GCN10_N_RASTERS; r++) {
        if (!selected(r, cond_mask, table_mask))
            continue;
        for (int k = 0; k < n_levels; k++) {
            p.out[r][k] = levels[q * n_levels + k];
            if (!p.out[r][k])
                return fail(GCN10_E_INVAL, "gcn10_gpu_overview_average: level %d of raster %d is NULL", k + 1, r);
        }
        q++;
    }
    const uint32_t W1 = ((uint32_t)W + 1u) >> 1;
    p.y1_begin = (uint32_t)y0 / 2u;
    p.y1_end = ((uint32_t)(y0 + rows) + 1u) / 2u;
    dim3 grid1((W1 + kThreads - 1) / kThreads, (p.y1_end - p.y1_begin + kL1Rows - 1) / kL1Rows);
    hipLaunchKernelGGL(overview_avg_level1_kernel, grid1, dim3(kThreads), 0, s, p);
    HIP_TRY(hipGetLastError());
    if (n_levels >= 2) {
        const uint32_t ty0 = (uint32_t)y0 / 256u, ty1 = ((uint32_t)(y0 + rows) + 255u) / 256u;
        dim3 grid2((W1 + kL1Tile - 1) / kL1Tile, ty1 - ty0, GCN10_N_RASTERS);
        hipLaunchKernelGGL(overview_avg_deeper_kernel, grid2, dim3(kThreads), 0, s, p, ty0);
        HIP_TRY(hipGetLastError());
    }
    return GCN10_OK;
}

}  // extern "C"
