// gcn10_soil_readers.hpp -- what every kernel that reads the soil of a prepared tile together with the landcover
// shares: the soil view, the all-tables lookup image, the 16-pixel gather and the raster selection test.  Readers:
// the strip kernels (gcn10_strip.hip), the fused encoder (gcn10_deflate_fused.hip), verify_strip (gcn10_verify.hip),
// the pair histograms (gcn10_stats.hip, gcn10_zonal.hip), the average overviews (gcn10_overview.hip), the area
// means (gcn10_aggregate.hip) and the sums on a model grid (gcn10_grid.hip, gcn10_grid_rain.hip, gcn10_zonal_rain.hip) and
// the strips through a byte table per cell (gcn10_runoff_strip.hip).  Their host side is gcn10::bind_soil / check_masks / grid_cap of
// gcn10_gpu_internal.hpp.
#ifndef GCN10_SOIL_READERS_HPP
#define GCN10_SOIL_READERS_HPP

#include "gcn10_gpu_internal.hpp"

namespace gcn10 {

// ---- the soil code bytes of the prepared tile, as a kernel sees them (filled by gcn10::bind_soil) -------------------
// hx[rows][stride]: one code byte per fine column (drained plane | undrained plane << 4); cj maps a row of the
// caller's strip to its coarse row.  cj comes from the caller (host-built, already clamped as src/cn.c:229 does); the
// clamp here only keeps a bad map from reading outside the workspace.
struct SoilView {
    const uint8_t *hx;      // null in a strip that reads the soil tables (codes, cx) instead
    const int32_t *cj;
    uint32_t stride, rows;

    // (also for a coarse row that came through the scalar cache or LDS)
    __device__ __forceinline__ uint32_t clamp(uint32_t r) const { return r < rows ? r : rows - 1u; }
    __device__ __forceinline__ uint32_t row(uint32_t y) const { return clamp((uint32_t)cj[y]); }
    // the code byte of column x in the (clamped) coarse row r, and of pixel (x, y) of the strip
    __device__ __forceinline__ const uint8_t *at(uint32_t r, uint32_t x) const { return hx + (size_t)r * stride + x; }
    __device__ __forceinline__ const uint8_t *ptr(uint32_t y, uint32_t x) const { return at(row(y), x); }
};

// ---- the all-tables lookup image (gcn10_gpu_ctx::d_lut16, written by gcn10_gpu_set_tables) --------------------------
// Six soil planes (0..4 and "invalid") of 256 rows of 16 bytes -- byte k = table k's value for (plane, landcover),
// 255 where there is none -- and one row of padding per plane, so that equal classes of different planes fall in
// different LDS banks.
constexpr int kPlanes = 6;
constexpr int kLut16Plane = 256 * 16 + 16;
constexpr int kLut16Bytes = kPlanes * kLut16Plane;
// The image of a single table k (gcn10_gpu_ctx::d_lut1 + k * kLut1Bytes): the same planes of one byte per landcover.
// LDS plane stride for the single-table byte LUT (+4 B pad: next bank).
constexpr int kPlane1 = 256 + 4;
constexpr int kLut1Bytes = kPlanes * kPlane1;

// the image into LDS, 16 bytes per thread and step (both 16-byte aligned); the caller synchronises
template <int THREADS>
__device__ __forceinline__ void stage_lut16(uint8_t *lds, const uint8_t *src)
{
    for (int i = threadIdx.x; i < kLut16Bytes / 16; i += THREADS)
        reinterpret_cast<u32x4 *>(lds)[i] = reinterpret_cast<const u32x4 *>(src)[i];
}

// the nine table values of (plane, landcover), and one of them
__device__ __forceinline__ const uint8_t *lut16_row(const uint8_t *lut, uint32_t plane, uint32_t lc)
{
    return lut + plane * (uint32_t)kLut16Plane + lc * 16u;
}

__device__ __forceinline__ uint32_t lut16_value(const uint8_t *lut, uint32_t plane, uint32_t lc, uint32_t k)
{
    return lut16_row(lut, plane, lc)[k];
}

// ---- 16 pixels of a lane against the image in LDS -----------------------------------------------------------------
// v_perm_b32: result byte i = byte sel[i] of the 8-byte pool {hi:lo} (selector 0..3 -> lo bytes 0..3, 4..7 -> hi bytes
// 0..3, 0x0c -> zero)
__device__ __forceinline__ uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
    return __builtin_amdgcn_perm(hi, lo, sel);
}

// 4x4 byte transpose: in a,b,c,d = one dword (4 table values) of pixels 0..3; out o[k] = {a.byte k, b.byte k,
// c.byte k, d.byte k} (pixel 0 in the low byte)
__device__ __forceinline__ void transpose4x4(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t &o0,
                                             uint32_t &o1, uint32_t &o2, uint32_t &o3)
{
    const uint32_t t0 = perm(b, a, 0x05010400u);    // a0 b0 a1 b1
    const uint32_t t1 = perm(b, a, 0x07030602u);    // a2 b2 a3 b3
    const uint32_t t2 = perm(d, c, 0x05010400u);    // c0 d0 c1 d1
    const uint32_t t3 = perm(d, c, 0x07030602u);    // c2 d2 c3 d3
    o0 = perm(t2, t0, 0x05040100u);                 // a0 b0 c0 d0
    o1 = perm(t2, t0, 0x07060302u);                 // a1 b1 c1 d1
    o2 = perm(t3, t1, 0x05040100u);                 // a2 b2 c2 d2
    o3 = perm(t3, t1, 0x07060302u);                 // a3 b3 c3 d3
}

__device__ __forceinline__ uint32_t gather_byte0(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const uint32_t t0 = perm(b, a, 0x0c0c0400u);    // a0 b0 0 0
    const uint32_t t1 = perm(d, c, 0x04000c0cu);    // 0 0 c0 d0
    return t0 | t1;
}

// The table values of a lane's 16 pixels (landcover e16, soil codes c16) for drainage condition `cond`:
// acc[k][j] = table k, pixels 4j .. 4j+3.  One ds_read_b128 per pixel, whatever the number of rasters wanted; the
// transposes turn "9 values of one pixel" into "4 pixels of one raster".  `cond` is a constant at every call (a
// template argument or the counter of an unrolled loop) and a plain argument all the same: picking one of two
// instantiations by that counter gave the strip kernels another schedule and up to 20 more registers.
__device__ __forceinline__ void gather16(const uint8_t *lut, const u32x4 &e16, const u32x4 &c16, const int cond,
                                         uint32_t acc[9][4])
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t e = e16[j], cd = c16[j];
        u32x4 r4[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t lc16 = q == 0 ? (e << 4) & 0xff0u : (e >> (8 * q - 4)) & 0xff0u;
            const uint32_t s = (cd >> (8 * q + 4 * cond)) & 0xfu;
            r4[q] = *reinterpret_cast<const u32x4 *>(lut + s * (uint32_t)kLut16Plane + lc16);
        }
        transpose4x4(r4[0][0], r4[1][0], r4[2][0], r4[3][0], acc[0][j], acc[1][j], acc[2][j], acc[3][j]);
        transpose4x4(r4[0][1], r4[1][1], r4[2][1], r4[3][1], acc[4][j], acc[5][j], acc[6][j], acc[7][j]);
        acc[8][j] = gather_byte0(r4[0][2], r4[1][2], r4[2][2], r4[3][2]);
    }
}

// ---- raster r = condition * 9 + table is wanted ---------------------------------------------------------------------
__host__ __device__ __forceinline__ bool selected(uint32_t r, uint32_t cond_mask, uint32_t table_mask)
{
    return (cond_mask >> (r / 9u)) & 1u && (table_mask >> (r % 9u)) & 1u;
}

}  // namespace gcn10

#endif
