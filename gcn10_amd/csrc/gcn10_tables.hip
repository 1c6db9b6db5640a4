// gcn10_tables.hip -- gcn10_gpu_set_tables: the lookup images every kernel gathers from, the pixel classes of the
// fused tile encoder, and the checks of the readers that depend on the loaded tables.
//
// Data layout in HBM:
//   lut16    [6][256] x 16 B     row (s, lc): bytes 0..8 = CN of tables 0..8,
//                                plane s=5 is all 255 (soil group not in 0..4)
//   lut1[k]  [6][256] x 1 B      the same for a single table k
// (strides and padding: kLut16Plane, kPlane1 of gcn10_soil_readers.hpp)

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "gcn10_gpu.h"
#include "gcn10_gpu_internal.hpp"
#include "gcn10_soil_readers.hpp"

using gcn10::fail;
using gcn10::kLut16Bytes;
using gcn10::kLut16Plane;
using gcn10::kLut1Bytes;
using gcn10::kPlane1;
using gcn10::use_device;

namespace gcn10 {

int check_tables(gcn10_gpu_ctx *ctx, const char *who)
{
    if (ctx->n_tables == 0)
        return fail(GCN10_E_STATE, "%s: call gcn10_gpu_set_tables first", who);
    return GCN10_OK;
}

int check_masks(gcn10_gpu_ctx *ctx, const char *who, unsigned cond_mask, unsigned table_mask)
{
    if (cond_mask == 0 || (cond_mask & ~3u))
        return fail(GCN10_E_INVAL, "%s: cond_mask 0x%x", who, cond_mask);
    if (table_mask == 0 || (table_mask >> ctx->n_tables))
        return fail(GCN10_E_INVAL, "%s: table_mask 0x%x with %d tables loaded", who, table_mask, ctx->n_tables);
    return GCN10_OK;
}

}  // namespace gcn10

namespace {

// Step 1: the all-tables image (left in img16 for step 2) and the nine single-table images, to the device.
int upload_lut_images(gcn10_gpu_ctx *ctx, const int *tables, int n_tables, uint8_t (&img16)[kLut16Bytes])
{
    static thread_local uint8_t img1[GCN10_N_TABLES * kLut1Bytes];
    memset(img16, GCN10_NODATA, sizeof img16);
    memset(img1, GCN10_NODATA, sizeof img1);
    for (int k = 0; k < n_tables; k++) {
        for (int lc = 0; lc < 256; lc++) {
            for (int s = 0; s < 5; s++) {
                const int v = tables[(k * 256 + lc) * 5 + s];
                // src/cn.c:125-128: only values < 255 are stored, through a
                // truncating (uint8_t) cast; everything else leaves the 255
                // the raster was memset to (src/cn.c:289).
                const uint8_t b = v < GCN10_NODATA ? (uint8_t)v : (uint8_t)GCN10_NODATA;
                img16[s * kLut16Plane + lc * 16 + k] = b;
                img1[k * kLut1Bytes + s * kPlane1 + lc] = b;
            }
        }
    }
    // synchronous copies: set_tables is a once-per-run call and the images are
    // reused by every later launch on any stream
    HIP_TRY(hipMemcpy(ctx->d_lut16, img16, sizeof img16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ctx->d_lut1, img1, sizeof img1, hipMemcpyHostToDevice));
    return GCN10_OK;
}

// Step 2: pixel classes for the fused tile encoder (gcn10_deflate_fused.hip): two pixels are in one
// class iff all 18 rasters agree on them, i.e. iff their (soil code, landcover) pairs have
// the same 18-vector of CN values.  Class 0 is the zero padding outside the raster.
int upload_pixel_classes(gcn10_gpu_ctx *ctx, int n_tables, const uint8_t (&img16)[kLut16Bytes])
{
    static thread_local uint8_t class_of[gcn10::kClassCodes * 256];
    static thread_local uint8_t class_val[GCN10_N_RASTERS * 256];
    static thread_local uint8_t vecs[257][GCN10_N_RASTERS];
    int n_classes = 1;
    memset(vecs[0], 0, sizeof vecs[0]);
    memset(class_val, 0, sizeof class_val);
    bool fits = true;
    for (int cc = 0; cc < gcn10::kClassCodes && fits; cc++) {
        const int sd = cc / 6, su = cc % 6;
        for (int lc = 0; lc < 256 && fits; lc++) {
            uint8_t v[GCN10_N_RASTERS];
            for (int r = 0; r < GCN10_N_RASTERS; r++) {
                const int sgrp = r < 9 ? sd : su;
                const int k = r % 9;
                v[r] = (sgrp < 5 && k < n_tables) ? img16[sgrp * kLut16Plane + lc * 16 + k]
                                                  : (uint8_t)GCN10_NODATA;
            }
            int id = -1;
            for (int c = 1; c < n_classes; c++)
                if (memcmp(vecs[c], v, sizeof v) == 0) {
                    id = c;
                    break;
                }
            if (id < 0) {
                if (n_classes == 256) {
                    fits = false;
                    break;
                }
                id = n_classes++;
                memcpy(vecs[id], v, sizeof v);
                for (int r = 0; r < GCN10_N_RASTERS; r++)
                    class_val[r * 256 + id] = v[r];
            }
            class_of[cc * 256 + lc] = (uint8_t)id;
        }
    }
    ctx->n_classes = fits ? n_classes : 0;      // 0: more than 256 classes, fused encoder unavailable
    if (fits) {
        if (!ctx->d_class_of)
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ctx->d_class_of), sizeof class_of + sizeof class_val));
        HIP_TRY(hipMemcpy(ctx->d_class_of, class_of, sizeof class_of, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(ctx->d_class_of + sizeof class_of, class_val, sizeof class_val,
                          hipMemcpyHostToDevice));
    }
    return GCN10_OK;
}

}  // namespace

extern "C" {

int gcn10_gpu_set_tables(gcn10_gpu_ctx *ctx, const int *tables, int n_tables)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (!tables || n_tables < 1 || n_tables > GCN10_N_TABLES)
        return fail(GCN10_E_INVAL, "gcn10_gpu_set_tables: need 1..9 tables, got %d", n_tables);

    static thread_local uint8_t img16[kLut16Bytes];
    if ((rc = upload_lut_images(ctx, tables, n_tables, img16)) != GCN10_OK)
        return rc;
    ctx->n_tables = n_tables;
    ctx->weights_set = false;       // the weight planes were folded from the tables before
    return upload_pixel_classes(ctx, n_tables, img16);
}

}  // extern "C"
