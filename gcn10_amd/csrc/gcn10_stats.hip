// gcn10_stats.hip -- the (landcover, soil code) pair histogram behind the band statistics of the outputs
// (config keys stats=1 / nodata=<v>, DESIGN.md "Band statistics").
//
// Every raster's value at a pixel is T8[k][landcover][plane], plane = the soil plane of the pixel for the
// condition (src/cn.c:88-131).  So one histogram per block over (landcover byte, soil code byte) pairs gives the
// exact histogram of all 18 rasters on the host, and no CN raster has to exist for it: the kernel reads the same
// inputs as cn_strip and the fused encoder, a landcover strip and the block's x-expanded soil codes.
//
// Only nine soil codes can occur (soil_code() of gcn10_device_util.hpp: planes 0..4 or 5 = invalid, drained = 4 for the
// dual classes), so the codes are mapped to a dense bin and a workgroup's private histogram is 16 x 256 dwords
// = 16 KiB of LDS.  Contention: in patchy landcover whole waves hit one bin, and 64 lanes adding to one LDS
// address serialise.  So every lane folds the runs of equal pairs of its 16 consecutive pixels in registers and
// adds one count per run; a wave whose 1024 pixels are all one pair adds once.  The workgroup histogram goes to
// the 64-bit device histogram once per workgroup, nonzero bins only.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gcn10_gpu_internal.hpp"
#include "gcn10_pair_hist.hpp"
#include "gcn10_soil_readers.hpp"

using namespace gcn10;
using namespace gcn10::pair_hist;

namespace {

constexpr uint32_t kChunk = kThreads * kPxPerLane;     // pixels of a row per workgroup step
constexpr uint32_t kRowsPerItem = 4;                   // rows of a workgroup step: 4 loads in flight per lane
// workgroups per CU at most; per 36000² block, patchy: 1 -> 1.55 ms, 2 -> 0.96, 4 -> 0.78, 8 -> 0.97
constexpr int kGridPerCu = 4;

struct HistParams {
    const uint8_t *esa;         // strip, W x rows, row major
    SoilView soil;              // x-expanded soil codes, soil row of every strip row
    unsigned long long *hist;   // [kBins][256]
    uint32_t W, rows, per_row;
};

__global__ __launch_bounds__(kThreads) void pair_histogram_kernel(const HistParams p)
{
    __shared__ uint32_t h[kHistWords];
    for (uint32_t i = threadIdx.x; i < (uint32_t)kHistWords; i += kThreads)
        h[i] = 0u;
    __syncthreads();

    // a workgroup step: kChunk pixels of kRowsPerItem rows; every lane has its rows' loads in flight together
    const uint64_t items = (uint64_t)((p.rows + kRowsPerItem - 1u) / kRowsPerItem) * p.per_row;
    for (uint64_t t = blockIdx.x; t < items; t += gridDim.x) {
        const uint32_t yg = (uint32_t)(t / p.per_row);
        const uint32_t x0 = (uint32_t)(t - (uint64_t)yg * p.per_row) * kChunk + threadIdx.x * kPxPerLane;
        const uint32_t y0 = yg * kRowsPerItem;
        const uint32_t ny = min(kRowsPerItem, p.rows - y0);        // wave uniform
        if (x0 >= p.W)
            continue;
        const uint8_t *erow[kRowsPerItem], *srow[kRowsPerItem];
#pragma unroll
        for (uint32_t j = 0; j < kRowsPerItem; j++) {
            const uint32_t y = y0 + min(j, ny - 1u);
            erow[j] = p.esa + (size_t)y * p.W + x0;
            srow[j] = p.soil.ptr(y, x0);
        }
        if (x0 + kPxPerLane <= p.W) {
            // 16 pixels inside the row: one 16-byte load of each (landcover rows start anywhere, soil rows on 16)
            typedef u32x4 u32x4_u __attribute__((aligned(1)));
            u32x4 e[kRowsPerItem], s[kRowsPerItem];
#pragma unroll
            for (uint32_t j = 0; j < kRowsPerItem; j++) {
                e[j] = *reinterpret_cast<const u32x4_u *>(erow[j]);
                s[j] = *reinterpret_cast<const u32x4 *>(srow[j]);
            }
#pragma unroll
            for (uint32_t j = 0; j < kRowsPerItem; j++)
                if (j < ny)
                    count16(h, e[j], s[j]);
        }
        else {
            for (uint32_t j = 0; j < ny; j++)
                count_tail(h, erow[j], srow[j], p.W - x0);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < (uint32_t)kHistWords; i += kThreads)
        if (h[i])
            atomicAdd(&p.hist[i], (unsigned long long)h[i]);
}

}  // namespace

extern "C" {

int gcn10_gpu_pair_histogram_codes(uint8_t codes[GCN10_PAIR_HIST_BINS])
{
    if (!codes)
        return fail(GCN10_E_INVAL, "gcn10_gpu_pair_histogram_codes: null pointer");
    for (int b = 0; b < kBins; b++)
        codes[b] = 0x55;                            // empty bins: the invalid plane in both conditions
    for (uint32_t d = 0; d <= 5; d++)
        codes[code_bin(d | d << 4)] = (uint8_t)(d | d << 4);
    for (uint32_t u = 1; u <= 3; u++)
        codes[code_bin(4u | u << 4)] = (uint8_t)(4u | u << 4);
    return GCN10_PAIR_HIST_BINS;
}

int gcn10_gpu_pair_histogram(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                             unsigned long long *hist_dev, gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    HistParams p = {};
    if ((rc = bind_soil(ctx, "gcn10_gpu_pair_histogram", W, as_stream(ctx, stream), cj, &p.soil)) != GCN10_OK)
        return rc;
    if (!esa || !cj || !hist_dev || W <= 0 || rows < 0)
        return fail(GCN10_E_INVAL, "gcn10_gpu_pair_histogram: bad arguments W=%d rows=%d", W, rows);
    if (rows == 0)
        return GCN10_OK;
    p.esa = esa;
    p.hist = hist_dev;
    p.W = (uint32_t)W;
    p.rows = (uint32_t)rows;
    p.per_row = ((uint32_t)W + kChunk - 1u) / kChunk;
    const uint64_t items = (uint64_t)((p.rows + kRowsPerItem - 1u) / kRowsPerItem) * p.per_row;
    const uint64_t cap = grid_cap(ctx, kGridPerCu);
    const uint32_t grid = (uint32_t)(items < cap ? items : cap);
    hipLaunchKernelGGL(pair_histogram_kernel, dim3(grid), dim3(kThreads), 0, as_stream(ctx, stream), p);
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}

}  // extern "C"
