// gcn10_reference_fns.hip -- the reference's three per-function steps as kernels of their own, on full-resolution
// rasters (the product's path is the fused strip, gcn10_strip.hip; these serve callers that port function by function).
//
// Reference behaviour restated here (citations are paths of the reference):
//   src/cn.c:218-232   HSG nearest-neighbour upsample  -> gcn10_gpu_resample
//   src/cn.c:88-111    modify_hysogs_data              -> gcn10_gpu_modify_hysogs_data
//   src/cn.c:114-131   calculate_cn                    -> gcn10_gpu_calculate_cn

#include <hip/hip_runtime.h>

#include <cstdint>

#include "gcn10_gpu.h"
#include "gcn10_device_util.hpp"
#include "gcn10_gpu_internal.hpp"
#include "gcn10_soil_readers.hpp"

using gcn10::aligned16;
using gcn10::as_stream;
using gcn10::fail;
using gcn10::first_chunk;
using gcn10::kInvalidPlane;
using gcn10::kLut1Bytes;
using gcn10::kPlane1;
using gcn10::kThreads;
using gcn10::load16_aligned_nt;
using gcn10::store16;
using gcn10::stream_grid;
using gcn10::u32x4;
using gcn10::use_device;

namespace {

__global__ __launch_bounds__(kThreads) void resample_rows(const uint8_t *coarse,
                                                          uint32_t hsx,
                                                          const int32_t *ci,
                                                          const int32_t *cj, uint32_t W,
                                                          uint32_t rows, uint8_t *out)
{
    const size_t npix = (size_t)W * rows;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += stride) {
        const uint32_t y = (uint32_t)(i / W);
        const uint32_t x = (uint32_t)(i - (size_t)y * W);
        out[i] = coarse[(size_t)(uint32_t)cj[y] * hsx + (uint32_t)ci[x]];   // src/cn.c:230
    }
}

// ------------------------------------------------------------------------
// modify_hysogs_data (src/cn.c:88-111), in place
// ------------------------------------------------------------------------
__device__ __forceinline__ uint8_t remap_soil(uint8_t h, bool drained)
{
    if (h >= 11 && h <= 14)
        return drained ? (uint8_t)4 : (uint8_t)(h - 10);
    return h;
}

__global__ __launch_bounds__(kThreads) void modify_hysogs_kernel(uint8_t *h, size_t npix,
                                                                 int drained,
                                                                 size_t head, size_t nvec)
{
    // [0, head) bytes, then nvec aligned 16-byte groups, then the tail bytes
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    u32x4 *body = reinterpret_cast<u32x4 *>(h + head);
    for (size_t v = tid; v < nvec; v += stride) {
        u32x4 in = body[v];
        u32x4 o;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            uint32_t w = 0;
#pragma unroll
            for (int q = 0; q < 4; q++)
                w |= (uint32_t)remap_soil((uint8_t)(in[j] >> (8 * q)), drained != 0) << (8 * q);
            o[j] = w;
        }
        body[v] = o;
    }
    const size_t tail0 = head + nvec * 16;
    const size_t nscalar = head + (npix - tail0);
    for (size_t s = tid; s < nscalar; s += stride) {
        const size_t i = s < head ? s : tail0 + (s - head);
        h[i] = remap_soil(h[i], drained != 0);
    }
}

// ------------------------------------------------------------------------
// calculate_cn (src/cn.c:114-131) on a full-resolution soil raster
// ------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kThreads) void calculate_cn_kernel(const uint8_t *esa,
                                                                const uint8_t *hsg,
                                                                size_t npix,
                                                                const uint8_t *lut_img,
                                                                uint8_t *out)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[kLut1Bytes];
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(lut_img);
        uint32_t *dst = reinterpret_cast<uint32_t *>(lut);
        for (int i = threadIdx.x; i < kLut1Bytes / 4; i += kThreads)
            dst[i] = src[i];
    }
    __syncthreads();

    const size_t nvec = VEC ? npix / 16 : 0;
    if (VEC) {
        // chunks of 2 x 256 vectors; every XCD streams a contiguous eighth (first_chunk)
        constexpr uint32_t kPer = 2;
        const uint32_t nchunks = (uint32_t)((nvec + kPer * kThreads - 1) / (kPer * kThreads));
        uint32_t step, end;
        for (uint32_t chunk = first_chunk(nchunks, step, end, true); chunk < end; chunk += step) {
            size_t v[kPer];
            u32x4 e16[kPer], h16[kPer];
            bool ok[kPer];
#pragma unroll
            for (uint32_t u = 0; u < kPer; u++) {
                v[u] = ((size_t)chunk * kPer + u) * kThreads + threadIdx.x;
                ok[u] = v[u] < nvec;
                const size_t at = ok[u] ? v[u] : 0;
                e16[u] = load16_aligned_nt(esa + at * 16);
                h16[u] = load16_aligned_nt(hsg + at * 16);
            }
#pragma unroll
            for (uint32_t u = 0; u < kPer; u++) {
                if (!ok[u])
                    continue;
                u32x4 o;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    uint32_t w = 0;
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const uint32_t lc = (e16[u][j] >> (8 * q)) & 0xffu;
                        uint32_t s = (h16[u][j] >> (8 * q)) & 0xffu;
                        s = s < 5u ? s : (uint32_t)kInvalidPlane;   // src/cn.c:123-124
                        w |= (uint32_t)lut[s * (uint32_t)kPlane1 + lc] << (8 * q);
                    }
                    o[j] = w;
                }
                store16(out + v[u] * 16, o);
            }
        }
    }
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t i = nvec * 16 + tid; i < npix; i += stride) {
        const uint32_t lc = esa[i];
        uint32_t s = hsg[i];
        s = s < 5u ? s : (uint32_t)kInvalidPlane;
        out[i] = lut[s * (uint32_t)kPlane1 + lc];
    }
}

}  // namespace

extern "C" {

int gcn10_gpu_resample(gcn10_gpu_ctx *ctx, const uint8_t *coarse, int hsx, int hsy,
                       const int32_t *ci, const int32_t *cj, int W, int rows, uint8_t *out,
                       gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (hsx <= 0 || hsy <= 0 || W < 0 || rows < 0)
        return fail(GCN10_E_INVAL, "gcn10_gpu_resample: bad shape %dx%d <- %dx%d", W, rows, hsx, hsy);
    if (W == 0 || rows == 0)
        return GCN10_OK;
    if (!coarse || !ci || !cj || !out)
        return fail(GCN10_E_INVAL, "gcn10_gpu_resample: null pointer");
    const uint64_t npix = (uint64_t)W * rows;
    const uint32_t grid = stream_grid(ctx, (npix + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(resample_rows, dim3(grid), dim3(kThreads), 0, as_stream(ctx, stream),
                       coarse, (uint32_t)hsx, ci, cj, (uint32_t)W, (uint32_t)rows, out);
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}

int gcn10_gpu_modify_hysogs_data(gcn10_gpu_ctx *ctx, uint8_t *h, size_t npix, int drained,
                                 gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (npix == 0)
        return GCN10_OK;
    if (!h)
        return fail(GCN10_E_INVAL, "gcn10_gpu_modify_hysogs_data: null pointer");
    size_t head = (16 - (reinterpret_cast<uintptr_t>(h) & 15u)) & 15u;
    if (head > npix)
        head = npix;
    const size_t nvec = (npix - head) / 16;
    const uint32_t grid = stream_grid(ctx, (nvec + kThreads - 1) / kThreads + 1);
    hipLaunchKernelGGL(modify_hysogs_kernel, dim3(grid), dim3(kThreads), 0,
                       as_stream(ctx, stream), h, npix, drained, head, nvec);
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}

int gcn10_gpu_calculate_cn(gcn10_gpu_ctx *ctx, const uint8_t *esa, const uint8_t *hsg,
                           size_t npix, int table_index, uint8_t *out, gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if ((rc = gcn10::check_tables(ctx, "gcn10_gpu_calculate_cn")) != GCN10_OK)
        return rc;
    if (table_index < 0 || table_index >= ctx->n_tables)
        return fail(GCN10_E_INVAL, "gcn10_gpu_calculate_cn: table %d not loaded (have %d)",
                    table_index, ctx->n_tables);
    if (npix == 0)
        return GCN10_OK;
    if (!esa || !hsg || !out)
        return fail(GCN10_E_INVAL, "gcn10_gpu_calculate_cn: null pointer");
    const uint8_t *img = ctx->d_lut1 + (size_t)table_index * kLut1Bytes;
    const bool vec = aligned16(esa) && aligned16(hsg) && aligned16(out);
    const uint64_t work = vec ? (npix / 16 + 2 * kThreads - 1) / (2 * kThreads) + 1
                              : (npix + kThreads - 1) / kThreads;
    const uint32_t grid = stream_grid(ctx, work);
    if (vec)
        hipLaunchKernelGGL(calculate_cn_kernel<true>, dim3(grid), dim3(kThreads), 0,
                           as_stream(ctx, stream), esa, hsg, npix, img, out);
    else
        hipLaunchKernelGGL(calculate_cn_kernel<false>, dim3(grid), dim3(kThreads), 0,
                           as_stream(ctx, stream), esa, hsg, npix, img, out);
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}

}  // extern "C"
