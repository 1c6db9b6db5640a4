// gcn10_strip.hip -- the strip kernels of the MI355X (gfx950 / CDNA4) curve-number engine: gcn10_gpu_cn_strip, the
// placement calibration gcn10_gpu_tune_single_raster and the plain copy they are measured against.
//
// Reference behaviour restated here (citations are paths of the reference):
//   src/cn.c:114-131   calculate_cn                    -> LDS table gather
//   src/cn.c:236-290   18 (cond, hc, arc) passes       -> one pass, 18 store streams
//
// Data layout in HBM (all rasters uint8, row-major, exactly the reference's
// malloc'd buffers, src/raster.c:169-178):
//   esa      [rows*W]            landcover strip, read once, 16 B / lane
//   out[r]   [rows*W]  r < 18    CN rasters, written once, 16 B / lane, nontemporal
// The soil comes from the prepared tile (gcn10_soil_tile.hip), the lookup images from gcn10_tables.hip.
//
// The dominant kernel (cn_strip_*) is HBM-bound: 1 + n_out bytes per pixel of
// DRAM traffic against ~20 VALU ops and 2 ds_read_b128 per pixel.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>

#include "gcn10_gpu.h"
#include "gcn10_device_util.hpp"
#include "gcn10_gpu_internal.hpp"
#include "gcn10_soil_readers.hpp"

using gcn10::aligned16;
using gcn10::as_stream;
using gcn10::fail;
using gcn10::first_chunk;
using gcn10::kChunk;
using gcn10::kLut16Bytes;
using gcn10::kLut1Bytes;
using gcn10::kPlane1;
using gcn10::kPxPerLane;
using gcn10::kThreads;
using gcn10::launch_timed;
using gcn10::load16_aligned;
using gcn10::load16_aligned_nt;
using gcn10::load16_any;
using gcn10::popcount;
using gcn10::scalar_load_i32;
using gcn10::SoilView;
using gcn10::store16;
using gcn10::stream_grid;
using gcn10::u32x4;
using gcn10::use_device;

namespace {

struct StripParams {
    const uint8_t *esa;
    SoilView soil;          // x-expanded soil codes (hx null when the strip reads the soil tables), coarse row of every strip row
    const uint8_t *lut;     // device image of the LDS table (lut16 or lut1[k])
    uint8_t *out[GCN10_N_RASTERS];
    uint32_t W;
    uint32_t rows;
    uint32_t npix;          // W*rows (< 2^31, as the reference's int npix, src/cn.c:208)
    uint32_t nvec16;        // npix rounded down to a multiple of 16: the part done in 16-byte lane groups
    uint32_t nchunks;
    uint32_t table_mask;
    uint32_t single_k;      // table index for the single-table variant
    uint32_t xcd_slabs;     // 1: each XCD streams a contiguous eighth of the strip
    // soil tables of the prepared tile (see soil_tables_kernel); codes = null: not in use, hx holds the bytes
    const uint32_t *cx;             // coarse column of every fine column
    const uint8_t *codes;           // soil code of every coarse cell, codes_stride bytes per coarse row
    uint32_t codes_stride;
    const uint32_t *soil_complex;    // device word: == soil_gen when some group of the tile has no compact form
    uint32_t soil_gen;               // generation number of the prepared tile (never 0)
};

// ------------------------------------------------------------------------
// cn_strip: the fused block kernel.
//
// KIND = kLut16 (all-tables): one 16-byte LDS row per (soil plane, class) holds
//   the CN of all nine tables, so a pixel costs one ds_read_b128 per drainage
//   condition whatever the number of rasters written; 4x4 byte transposes
//   (v_perm_b32) turn "9 values of one pixel" into "4 pixels of one raster".
// KIND = kLut1 (single table, BASELINE config 2): 2 B/px of HBM traffic, so the
//   pixel rate is ~8x higher and the LDS work per pixel is one byte read.
// ILP  = 1024-px wave chunks a wave handles per loop trip; all their loads are
//   issued before any is consumed.
// NT   = nontemporal landcover loads and raster stores.
// PF   = software pipeline: the loads of trip t+1 are issued before trip t's
//   gathers and stores, on two register sets used alternately (vmcnt counts
//   loads and stores in one in-order queue on gfx950, so a wave that loads,
//   stores, loads ... has nothing in flight while it gathers; with the next
//   trip's loads issued first, its stores and those loads overlap).
//
// The loop body has no divergent region: a raster is processed as a flat byte
// array in 16-byte lane groups, every lane of every wave issues the same loads,
// and the three irregular cases are folded in without a branch that holds
// memory operations --
//   * lanes past the last full 16-byte group load from offset 0 and skip the
//     store (exec mask on the store only); the npix % 16 tail pixels are done
//     byte-wise after the loop;
//   * lanes behind a row end inside the wave's 1024-px span use the next
//     raster row's soil row (both coarse rows come through the scalar cache);
//   * only when W % 16 != 0 can a lane's 16 pixels straddle a row end: the
//     wave that holds such a lane (a scalar test, one wave in ~35) issues a
//     second soil load for it that starts n bytes before the next soil row, and
//     merges the two vectors with byte masks.
// Requires W >= kMinVectorW so that a wave's span wraps at most once.
// ------------------------------------------------------------------------
enum { kLut16 = 0, kLut1 = 1 };
constexpr uint32_t kWavePx = 64u * kPxPerLane;      // 1024 px per wave chunk
constexpr uint32_t kMinVectorW = kWavePx + 16u;

// Where a strip kernel takes the soil codes of a lane's 16 pixels from.
//   kSoilBytes:  the code bytes of the hx workspace (any W)
//   kSoilLanes:  W % 16 == 0, so the 16 pixels are one column group, and the lane keeps that group for the whole
//                launch (gcn10::strip_lane_plan): its column entry {c_lo, c_hi, split} is made once, a trip loads
//                the two codes of its coarse row from the codes table
//   kSoilPixels: the codes table through the column map, pixel by pixel, for a tile with a group that has no
//                compact entry (the same lane plan)
enum { kSoilBytes = 0, kSoilLanes = 1, kSoilPixels = 2 };

// What a lane holds of one trip between issuing its loads and using them.
template <int ILP>
struct Trip {
    u32x4 e16[ILP], c16[ILP];
    uint32_t i0[ILP];
};

// The loads of one trip of a strip that reads the code bytes: chunks of 4096 px dealt by first_chunk.
template <int ILP, bool NT>
__device__ __forceinline__ void issue_trip(const StripParams &p, uint32_t trip, uint32_t lane_off,
                                           uint32_t wave_off, Trip<ILP> &tr)
{
    // ---- wave-uniform part: row and column of the wave's first pixel, the coarse rows of that
    // raster row and of the next one through the scalar cache (s_load, own counter) ----
    uint32_t xb[ILP], r0[ILP], r1[ILP], wb[ILP];
#pragma unroll
    for (int u = 0; u < ILP; u++) {
        wb[u] = __builtin_amdgcn_readfirstlane((trip * ILP + u) * (uint32_t)kChunk + wave_off);
        const uint32_t wbc = wb[u] < p.npix ? wb[u] : 0u;   // a wave past the end only needs valid addresses
        const uint32_t y = wbc / p.W;
        xb[u] = wbc - y * p.W;
        r0[u] = (uint32_t)scalar_load_i32(p.soil.cj, y);
        r1[u] = (uint32_t)scalar_load_i32(p.soil.cj, y + 1u < p.rows ? y + 1u : y);
    }
#pragma unroll
    for (int u = 0; u < ILP; u++) {
        tr.i0[u] = wb[u] + lane_off;
        const uint8_t *pe = p.esa + (tr.i0[u] < p.nvec16 ? tr.i0[u] : 0u);
        tr.e16[u] = NT ? load16_aligned_nt(pe) : load16_aligned(pe);
    }
#pragma unroll
    for (int u = 0; u < ILP; u++) {
        uint32_t xl = xb[u] + lane_off;
        const bool wrap = xl >= p.W;
        xl = wrap ? xl - p.W : xl;
        const uint32_t row = p.soil.clamp(wrap ? r1[u] : r0[u]);
        const uint8_t *pa = p.soil.at(row, xl);
        u32x4 a = load16_any(pa);
        if (p.W & 15u) {
            const uint32_t n = p.W - xl;            // pixels of this lane that are still in its row
            const bool strad = !wrap && n < (uint32_t)kPxPerLane;
            if (__builtin_amdgcn_ballot_w64(strad) != 0ull) {
                // the other lanes of this wave re-read their own vector (an L1 hit)
                const uint8_t *pb = strad ? p.soil.at(p.soil.clamp(r1[u]), 0u) - n : pa;
                const u32x4 b = load16_any(pb);
                const uint32_t nn = strad ? n : (uint32_t)kPxPerLane;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int32_t m = (int32_t)nn - 4 * j;      // bytes of dword j that come from a
                    const uint32_t mask = m >= 4 ? 0xffffffffu : (m <= 0 ? 0u : (1u << (8 * m)) - 1u);
                    a[j] = (a[j] & mask) | (b[j] & ~mask);
                }
            }
        }
        tr.c16[u] = a;
    }
}

// ---- strips that read the soil tables: one column group per lane (gcn10::strip_lane_plan) ----
// What such a lane keeps for the whole launch.
struct LaneSoil {
    uint32_t base;          // pixel index of the lane's vector in sub-trip 0
    uint32_t lim;           // end of the lane's piece in pixels; 0 for a lane without a column group
    uint32_t sub_px;        // pixels per sub-trip (B rows), wave-uniform
    uint32_t y_first;       // strip row of the wave's first lane in sub-trip 0, wave-uniform
    uint32_t B;
    bool wrap;              // the lane is behind the row end inside its wave: one row further than the first lane
    uint32_t x;             // first fine column of the group
    uint32_t c_lo, c_hi;    // coarse columns of the group's first and last pixel
    int32_t split;          // pixels [0, split) of the 16 take the code of c_lo, the rest that of c_hi
    uint32_t mask[4];       // the same as byte masks of the four dwords (single-table kernel: see mix_lane_codes)
    bool pair;              // wave-uniform: c_hi is c_lo or c_lo + 1 in every lane, one 2-byte load fetches both codes
};

// byte mask of dword j of a lane's 16 pixels: the bytes of the pixels below `split`
__device__ __forceinline__ uint32_t split_mask(int32_t split, int j)
{
    const int32_t m = split - 4 * j;
    return m >= 4 ? 0xffffffffu : (m <= 0 ? 0u : (1u << (8 * m)) - 1u);
}

template <int SOIL>
__device__ __forceinline__ void lane_prologue(const StripParams &p, const gcn10::StripLanePlan &pl, LaneSoil &ls)
{
    const uint32_t g_first = __builtin_amdgcn_readfirstlane(pl.g);
    ls.base = (pl.row_lo * pl.G + pl.t) * (uint32_t)kPxPerLane;
    ls.lim = pl.active ? pl.row_hi * p.W : 0u;
    ls.sub_px = pl.B * p.W;
    ls.y_first = pl.row_lo + __builtin_amdgcn_readfirstlane(pl.rho);
    ls.B = pl.B;
    ls.wrap = pl.g < g_first;
    ls.x = pl.g * (uint32_t)kPxPerLane;
    ls.c_lo = ls.c_hi = 0u;
    ls.split = 16;
    ls.pair = true;
    if (SOIL == kSoilLanes) {
        // the column entry, by the rule of soil_tables_kernel: a run of c_lo, then c_hi (cx is already clamped)
        uint32_t cx[16];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const u32x4 c4 = *reinterpret_cast<const u32x4 *>(p.cx + ls.x + 4 * j);
#pragma unroll
            for (int q = 0; q < 4; q++)
                cx[4 * j + q] = c4[q];
        }
        ls.c_lo = cx[0];
        ls.c_hi = cx[15];
        uint32_t split = 0;
#pragma unroll
        for (int q = 0; q < 16; q++)
            split += cx[q] == ls.c_lo && split == (uint32_t)q ? 1u : 0u;
        ls.split = (int32_t)split;
#pragma unroll
        for (int j = 0; j < 4; j++)
            ls.mask[j] = split_mask(ls.split, j);
        // (a row of codes ends with a padding code: the byte behind c_lo exists)
        ls.pair = __builtin_amdgcn_ballot_w64(ls.c_hi - ls.c_lo > 1u) == 0ull;
    }
}

template <int ILP, bool NT, int SOIL>
__device__ __forceinline__ void issue_lane_trip(const StripParams &p, const LaneSoil &ls, uint32_t trip,
                                                Trip<ILP> &tr)
{
    // ---- wave-uniform part: the strip row of the wave's first lane, its coarse row and the next row's through the
    // scalar cache (s_load, own counter), as offsets into the codes table ----
    uint32_t o0[ILP], o1[ILP];
#pragma unroll
    for (int u = 0; u < ILP; u++) {
        const uint32_t y = ls.y_first + (trip * ILP + u) * ls.B;
        const uint32_t ya = y < p.rows ? y : p.rows - 1u;       // a wave past the end only needs valid addresses
        const uint32_t yb = y + 1u < p.rows ? y + 1u : p.rows - 1u;
        o0[u] = p.soil.clamp((uint32_t)scalar_load_i32(p.soil.cj, ya)) * p.codes_stride;
        o1[u] = p.soil.clamp((uint32_t)scalar_load_i32(p.soil.cj, yb)) * p.codes_stride;
    }
#pragma unroll
    for (int u = 0; u < ILP; u++) {
        const uint32_t i0 = ls.base + (trip * ILP + u) * ls.sub_px;
        const bool live = i0 < ls.lim;
        tr.i0[u] = live ? i0 : 0xffffffffu;                     // (finish_trip: not below nvec16, no store)
        const uint8_t *pe = p.esa + (live ? i0 : 0u);
        tr.e16[u] = NT ? load16_aligned_nt(pe) : load16_aligned(pe);
    }
#pragma unroll
    for (int u = 0; u < ILP; u++) {
        const uint32_t off = ls.wrap ? o1[u] : o0[u];
        if (SOIL == kSoilLanes) {
            typedef uint16_t u16_u __attribute__((aligned(1)));
            tr.c16[u][0] = *reinterpret_cast<const u16_u *>(p.codes + (off + ls.c_lo));
            if (!ls.pair)
                tr.c16[u][1] = p.codes[off + ls.c_hi];
        }
        else {
            // rare (a tile with fewer than 8 columns per soil cell, a map that is not monotone): asked to be right,
            // not fast -- a rolled loop, so that it adds nothing to the registers of the kernel
            const uint8_t *cr = p.codes + off;
            const u32x4 *pc = reinterpret_cast<const u32x4 *>(p.cx + ls.x);
            u32x4 a = { 0u, 0u, 0u, 0u };
#pragma unroll 1
            for (int j = 0; j < 4; j++) {
                const u32x4 c4 = pc[j];
                const uint32_t w = (uint32_t)cr[c4[0]] | (uint32_t)cr[c4[1]] << 8 | (uint32_t)cr[c4[2]] << 16 |
                                   (uint32_t)cr[c4[3]] << 24;
                a[0] = j == 0 ? w : a[0];
                a[1] = j == 1 ? w : a[1];
                a[2] = j == 2 ? w : a[2];
                a[3] = j == 3 ? w : a[3];
            }
            tr.c16[u] = a;
        }
    }
}

// Soil code bytes of a lane's 16 pixels from the two codes of its column entry: pixels [0, split) have the code of
// c_lo, the rest the code of c_hi.  KEEP_MASKS: the four byte masks are registers of the whole launch (the
// single-table kernel has them to spare).  Else they are made again from `split` for every vector, and the compiler
// is kept from hoisting them: with the masks loop-invariant it also hoists what the all-tables gather derives from
// them, 20 to 30 VGPRs and a wave per SIMD in the pipelined variants.
template <bool KEEP_MASKS>
__device__ __forceinline__ u32x4 mix_lane_codes(const LaneSoil &ls, const u32x4 &c)
{
    const uint32_t a = (c[0] & 0xffu) * 0x01010101u;
    const uint32_t b = (ls.pair ? (c[0] >> 8) & 0xffu : c[1] & 0xffu) * 0x01010101u;
    u32x4 cd;
    int32_t split = ls.split;
    if (!KEEP_MASKS)
        asm volatile("" : "+v"(split));
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t mask = KEEP_MASKS ? ls.mask[j] : split_mask(split, j);
        cd[j] = (a & mask) | (b & ~mask);
    }
    return cd;
}

// Table gathers and stores of one trip.
template <int KIND, int COND_MASK, int ILP, bool NT, int SOIL>
__device__ __forceinline__ void finish_trip(const StripParams &p, const uint8_t *lut, uint32_t tmask,
                                            const Trip<ILP> &tr, const LaneSoil &ls)
{
#pragma unroll
    for (int u = 0; u < ILP; u++) {
        const bool live = tr.i0[u] < p.nvec16;
        const u32x4 c16 = SOIL == kSoilLanes ? mix_lane_codes<KIND == kLut1>(ls, tr.c16[u]) : tr.c16[u];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            if (!(COND_MASK & (1 << c)))
                continue;
            if (KIND == kLut16) {
                uint32_t acc[9][4];
                gcn10::gather16(lut, tr.e16[u], c16, c, acc);
                if (live) {
#pragma unroll
                    for (int k = 0; k < 9; k++) {
                        if (tmask & (1u << k)) {
                            u32x4 v = {acc[k][0], acc[k][1], acc[k][2], acc[k][3]};
                            store16<NT>(p.out[c * 9 + k] + tr.i0[u], v);
                        }
                    }
                }
            }
            else {
                u32x4 v;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint32_t e = tr.e16[u][j];
                    const uint32_t cd = c16[j];
                    uint32_t w = 0;
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const uint32_t lc = (e >> (8 * q)) & 0xffu;
                        const uint32_t s = (cd >> (8 * q + 4 * c)) & 0xfu;
                        const uint32_t b = lut[s * (uint32_t)kPlane1 + lc];
                        w |= b << (8 * q);
                    }
                    v[j] = w;
                }
                if (live)
                    store16<NT>(p.out[c * 9 + p.single_k] + tr.i0[u], v);
            }
        }
    }
}

// The trip loop of cn_strip_kernel.  SOIL == kSoilBytes: trips are groups of ILP chunks of 4096 px, dealt by
// first_chunk (p.nchunks counts them).  Else: the trips of the lane plan, every lane in its column group.
template <int KIND, int COND_MASK, int ILP, bool NT, bool PF, int SOIL>
__device__ __forceinline__ void strip_loop(const StripParams &p, const uint8_t *lut, uint32_t tmask)
{
    uint32_t step = 1u, end, trip = 0u, lane_off = 0u, wave_off = 0u;
    LaneSoil ls = {};
    if (SOIL == kSoilBytes) {
        lane_off = (threadIdx.x & 63u) * kPxPerLane;
        wave_off = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * kWavePx;
        trip = first_chunk(p.nchunks, step, end, p.xcd_slabs != 0);
    }
    else {
        const gcn10::StripLanePlan pl = gcn10::strip_lane_plan(p.W, p.rows, gridDim.x, blockIdx.x, threadIdx.x,
                                                               p.xcd_slabs != 0, (uint32_t)ILP);
        end = __builtin_amdgcn_readfirstlane(pl.trips);
        // (lane numbers rise within a wave: its first lane has a column group or none has)
        if (!__builtin_amdgcn_readfirstlane((uint32_t)pl.active))
            return;
        lane_prologue<SOIL>(p, pl, ls);
    }
    if (trip >= end)
        return;
    auto issue = [&](uint32_t t, Trip<ILP> &tr) {
        if (SOIL == kSoilBytes)
            issue_trip<ILP, NT>(p, t, lane_off, wave_off, tr);
        else
            issue_lane_trip<ILP, NT, SOIL>(p, ls, t, tr);
    };
    if (!PF) {
        for (; trip < end; trip += step) {
            Trip<ILP> tr;
            issue(trip, tr);
            finish_trip<KIND, COND_MASK, ILP, NT, SOIL>(p, lut, tmask, tr, ls);
        }
    }
    else {
        Trip<ILP> ta, tb;       // used alternately: a copy would wait for the loads it copies
        issue(trip, ta);
        for (;;) {
            trip += step;
            if (trip >= end) {
                finish_trip<KIND, COND_MASK, ILP, NT, SOIL>(p, lut, tmask, ta, ls);
                break;
            }
            issue(trip, tb);
            finish_trip<KIND, COND_MASK, ILP, NT, SOIL>(p, lut, tmask, ta, ls);
            trip += step;
            if (trip >= end) {
                finish_trip<KIND, COND_MASK, ILP, NT, SOIL>(p, lut, tmask, tb, ls);
                break;
            }
            issue(trip, ta);
            finish_trip<KIND, COND_MASK, ILP, NT, SOIL>(p, lut, tmask, tb, ls);
        }
    }
}

template <int KIND, int COND_MASK, bool ALL_TABLES, int ILP, bool NT, bool PF>
__global__ __launch_bounds__(kThreads) void cn_strip_kernel(const StripParams p)
{
    constexpr int kLutBytes = KIND == kLut16 ? kLut16Bytes : kLut1Bytes;
    __shared__ __attribute__((aligned(16))) uint8_t lut[kLutBytes];

    if (KIND == kLut16) {
        gcn10::stage_lut16<kThreads>(lut, p.lut);
    }
    else {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(p.lut);
        uint32_t *dst = reinterpret_cast<uint32_t *>(lut);
        for (int i = threadIdx.x; i < kLutBytes / 4; i += kThreads)
            dst[i] = src[i];
    }
    __syncthreads();

    const uint32_t tmask = ALL_TABLES ? 0x1ffu : p.table_mask;

    // the soil tables when the host offers them: a column entry per lane, or the codes table pixel by pixel when some
    // group of this tile is complex (wave-uniform: the flag comes through the scalar cache); else the code bytes
    if (!p.codes)
        strip_loop<KIND, COND_MASK, ILP, NT, PF, kSoilBytes>(p, lut, tmask);
    else if ((uint32_t)scalar_load_i32(reinterpret_cast<const int32_t *>(p.soil_complex), 0u) != p.soil_gen)
        strip_loop<KIND, COND_MASK, ILP, NT, PF, kSoilLanes>(p, lut, tmask);
    else
        strip_loop<KIND, COND_MASK, ILP, NT, PF, kSoilPixels>(p, lut, tmask);

    // the last npix % 16 pixels, one per thread
    if (blockIdx.x == 0 && threadIdx.x < p.npix - p.nvec16) {
        const uint32_t i = p.nvec16 + threadIdx.x;
        const uint32_t y = i / p.W;
        const uint32_t x = i - y * p.W;
        const uint32_t lc = p.esa[i];
        // (a strip that reads the soil tables has W % 16 == 0, so no tail: p.soil.hx is set whenever this runs)
        const uint32_t cd = *p.soil.ptr(y, x);
#pragma unroll
        for (int c = 0; c < 2; c++) {
            if (!(COND_MASK & (1 << c)))
                continue;
            const uint32_t s = (cd >> (4 * c)) & 0xfu;
            if (KIND == kLut16) {
                const uint8_t *row = gcn10::lut16_row(lut, s, lc);
                for (int k = 0; k < 9; k++)
                    if (tmask & (1u << k))
                        p.out[c * 9 + k][i] = row[k];
            }
            else {
                p.out[c * 9 + p.single_k][i] = lut[s * (uint32_t)kPlane1 + lc];
            }
        }
    }
}

// ------------------------------------------------------------------------
// plain 1R:1W copy with the strip kernel's launch shape (XCD slabs, 16 B per
// lane, two chunks per trip, nontemporal): what this device streams when a
// kernel does nothing but move the bytes.  bench.py times it in the same run
// as the strip kernel (gcn10_gpu_stream_copy).
// ------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void stream_copy_kernel(const u32x4 *in, u32x4 *out, uint32_t nvec,
                                                               uint32_t ntrips)
{
    uint32_t step, end;
    for (uint32_t trip = first_chunk(ntrips, step, end, true); trip < end; trip += step) {
        u32x4 v[2];
        uint32_t idx[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            idx[u] = (trip * 2u + u) * (uint32_t)kThreads + threadIdx.x;
            v[u] = __builtin_nontemporal_load(in + (idx[u] < nvec ? idx[u] : 0u));
        }
#pragma unroll
        for (int u = 0; u < 2; u++)
            if (idx[u] < nvec)
                __builtin_nontemporal_store(v[u], out + idx[u]);
    }
}

// ------------------------------------------------------------------------
// byte-wise strip kernel: any alignment, any shape.  Used when a raster
// pointer is not 16-byte aligned (never the case for the host pipeline).
// ------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void cn_strip_bytes(const StripParams p,
                                                           uint32_t cond_mask)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[kLut16Bytes];
    gcn10::stage_lut16<kThreads>(lut, p.lut);
    __syncthreads();

    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < p.npix; i += stride) {
        const uint32_t y = i / p.W;
        const uint32_t x = i - y * p.W;
        const uint32_t lc = p.esa[i];
        const uint32_t cd = *p.soil.ptr(y, x);
        for (int c = 0; c < 2; c++) {
            if (!(cond_mask & (1u << c)))
                continue;
            const uint32_t s = (cd >> (4 * c)) & 0xfu;
            const uint8_t *row = gcn10::lut16_row(lut, s, lc);
            for (int k = 0; k < 9; k++)
                if (p.table_mask & (1u << k))
                    p.out[c * 9 + k][i] = row[k];
        }
    }
}

// ------------------------------------------------------------------------
// The strip-kernel table: every cn_strip_kernel instantiation the library carries, with the name rocprofv3 prints
// for it (gcn10_gpu_last_kernel_name; bench.py and the tests read it).  A row makes the function pointer and the
// name from the same six template arguments, written as literals: KIND 0 = kLut16, 1 = kLut1.
//   all-tables kind:  COND_MASK 1..3 x ALL_TABLES x ILP 1, 2 x NT x PF          48
//   single table:     COND_MASK 1..3 x ILP 1, 2 x NT x PF, and ILP 4 x NT        30
// ------------------------------------------------------------------------
typedef void (*strip_kernel_t)(const StripParams);

struct StripKernel {
    int kind, cond_mask;
    bool all_tables;
    int ilp;
    bool nt, pf;
    strip_kernel_t fn;
    const char *name;
};

#define STRIP_ROW(K, C, A, I, N, P)                          \
    { K, C, A, I, N, P, cn_strip_kernel<K, C, A, I, N, P>,   \
      "cn_strip_kernel<" #K ", " #C ", " #A ", " #I ", " #N ", " #P ">" },
#define STRIP_NT_ROWS(K, C, A, I, P) STRIP_ROW(K, C, A, I, false, P) STRIP_ROW(K, C, A, I, true, P)
#define STRIP_ILP_ROWS(K, C, A)                                        \
    STRIP_NT_ROWS(K, C, A, 1, false) STRIP_NT_ROWS(K, C, A, 1, true)   \
    STRIP_NT_ROWS(K, C, A, 2, false) STRIP_NT_ROWS(K, C, A, 2, true)
#define STRIP_COND_ROWS(K, A) STRIP_ILP_ROWS(K, 1, A) STRIP_ILP_ROWS(K, 2, A) STRIP_ILP_ROWS(K, 3, A)

const StripKernel kStripKernels[] = {
    STRIP_COND_ROWS(0, false) STRIP_COND_ROWS(0, true)
    STRIP_COND_ROWS(1, true)
    STRIP_NT_ROWS(1, 1, true, 4, false) STRIP_NT_ROWS(1, 2, true, 4, false) STRIP_NT_ROWS(1, 3, true, 4, false)
};
static_assert(sizeof kStripKernels / sizeof kStripKernels[0] == 78, "the library carries 78 strip kernels");
static_assert(kLut16 == 0 && kLut1 == 1, "KIND of the rows above");

#undef STRIP_COND_ROWS
#undef STRIP_ILP_ROWS
#undef STRIP_NT_ROWS
#undef STRIP_ROW

// The kernel of a request, or null when there is none (ILP 4 of the all-tables kind, an ILP other than 1, 2, 4).
// The folding rules live here and nowhere else.
// (the pipeline choice `pf` is an argument: two worker threads pick kernels for their own contexts at the same time,
// a process-wide flag would be a data race)
const StripKernel *find_strip_kernel(bool single, unsigned cond_mask, bool all, int ilp, bool nt, bool pf)
{
    const int kind = single ? kLut1 : kLut16;
    all = all || single;        // the single-table kernel ignores ALL_TABLES: instantiated once
    pf = pf && ilp <= 2;        // pipelined variants exist for ILP 1 and 2 (two register sets of ILP 4 cost occupancy)
    for (const StripKernel &k : kStripKernels)
        if (k.kind == kind && k.cond_mask == (int)cond_mask && k.all_tables == all && k.ilp == ilp && k.nt == nt &&
            k.pf == pf)
            return &k;
    return nullptr;
}

}  // namespace

extern "C" {

int gcn10_gpu_cn_strip(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows,
                       const int32_t *cj, unsigned cond_mask, unsigned table_mask,
                       uint8_t *const out[GCN10_N_RASTERS], gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    const char *const who = "gcn10_gpu_cn_strip";
    if ((rc = gcn10::check_tables(ctx, who)) != GCN10_OK || (rc = gcn10::check_tile(ctx, who)) != GCN10_OK)
        return rc;
    // (a width other than the prepared tile's is a bad argument here, a bad state to the other readers)
    if (W <= 0 || rows < 0 || (uint32_t)W != ctx->tile.hx_W)
        return fail(GCN10_E_INVAL, "gcn10_gpu_cn_strip: W=%d rows=%d does not match prepared tile W=%u",
                    W, rows, ctx->tile.hx_W);
    if ((uint64_t)W * (uint64_t)rows > 0x7fffffffull)
        return fail(GCN10_E_INVAL, "gcn10_gpu_cn_strip: strip of %d x %d exceeds 2^31-1 pixels", W, rows);
    if ((rc = gcn10::check_masks(ctx, who, cond_mask, table_mask)) != GCN10_OK)
        return rc;
    if (rows == 0)
        return GCN10_OK;
    if (!esa || !cj || !out)
        return fail(GCN10_E_INVAL, "gcn10_gpu_cn_strip: null pointer");

    StripParams p;
    memset(&p, 0, sizeof p);
    bool all_aligned = aligned16(esa);
    for (int r = 0; r < GCN10_N_RASTERS; r++) {
        if (!gcn10::selected(r, cond_mask, table_mask))
            continue;
        if (!out[r])
            return fail(GCN10_E_INVAL, "gcn10_gpu_cn_strip: out[%d] is null but selected", r);
        p.out[r] = out[r];
        all_aligned = all_aligned && aligned16(out[r]);
    }
    p.esa = esa;
    p.W = (uint32_t)W;
    p.rows = (uint32_t)rows;
    p.npix = (uint32_t)((uint64_t)W * (uint64_t)rows);
    p.nchunks = (p.npix + kChunk - 1) / kChunk;
    p.table_mask = table_mask;
    hipStream_t s = as_stream(ctx, stream);

    p.xcd_slabs = (uint32_t)ctx->opt.xcd_slabs;
    p.nvec16 = p.npix & ~15u;
    // the vector kernel wants a wave's 1024-px span to cross at most one row end
    if (p.npix < 16u || p.W < kMinVectorW)
        all_aligned = false;
    // the launch shape of the vector kernel (needed here: whether a strip can read the soil tables depends on it)
    const bool single = popcount(table_mask) == 1;
    const bool tuned = single && ctx->opt.single.set;
    // 0 = by the number of store streams: two chunks per trip up to nine rasters, one beyond
    const int n_streams = popcount(cond_mask) * popcount(table_mask);
    const int ilp = tuned ? ctx->opt.single.ilp
                          : single ? ctx->opt.ilp1 : (ctx->opt.ilp16 > 0 ? ctx->opt.ilp16 : (n_streams > 9 ? 1 : 2));
    p.nchunks = (p.nchunks + (uint32_t)ilp - 1) / (uint32_t)ilp;    // groups of ILP sub-chunks
    const uint32_t grid = stream_grid(ctx, p.nchunks, tuned ? ctx->opt.single.grid_blocks_per_cu : 0);
    if (tuned)
        p.xcd_slabs = (uint32_t)ctx->opt.single.xcd_slabs;
    // rows are 16-byte aligned: a lane's 16 pixels are one column group, and the lane plan keeps it there -- unless
    // a row has more column groups than the grid has threads (a very wide strip on a small grid: the code bytes)
    if (all_aligned && ctx->opt.compact_soil && (p.W & 15u) == 0u &&
        gcn10::strip_lane_plan(p.W, p.rows, grid, 0u, 0u, p.xcd_slabs != 0, (uint32_t)ilp).B > 0u) {
        p.soil = SoilView{ nullptr, cj, ctx->tile.hx_stride, ctx->tile.hx_rows };
        p.cx = ctx->tile.d_cx;
        p.codes = ctx->tile.d_codes;
        p.codes_stride = ctx->tile.codes_stride;
        p.soil_complex = ctx->tile.d_soil_complex;
        p.soil_gen = ctx->tile.soil_gen;
    }
    else {
        rc = gcn10::bind_soil(ctx, who, W, s, cj, &p.soil);
        if (rc)
            return rc;
    }
    if (!all_aligned) {
        p.lut = ctx->d_lut16;
        const uint32_t g = stream_grid(ctx, ((uint64_t)p.npix + kThreads - 1) / kThreads);
        void *args[] = { &p, &cond_mask };
        HIP_TRY(launch_timed(ctx, reinterpret_cast<const void *>(cn_strip_bytes), g, args, s));
        ctx->last_kernel = "cn_strip_bytes";
    }
    else {
        if (single) {
            p.single_k = (uint32_t)__builtin_ctz(table_mask);
            p.lut = ctx->d_lut1 + (size_t)p.single_k * kLut1Bytes;
        }
        else {
            p.lut = ctx->d_lut16;
        }
        const StripKernel *k = find_strip_kernel(single, cond_mask, table_mask == 0x1ffu, ilp, ctx->opt.nontemporal != 0,
                                                 (tuned ? ctx->opt.single.prefetch : ctx->opt.prefetch) != 0);
        if (!k)
            return fail(GCN10_E_INVAL, "gcn10_gpu_cn_strip: no kernel for ilp=%d", ilp);
        void *args[] = { &p };
        HIP_TRY(launch_timed(ctx, reinterpret_cast<const void *>(k->fn), grid, args, s));
        ctx->last_kernel = k->name;
    }
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}

size_t gcn10_gpu_strip_algorithmic_bytes(int W, int rows, int hsx, int hsy, unsigned cond_mask,
                                         unsigned table_mask)
{
    if (W <= 0 || rows <= 0)
        return 0;
    const size_t n_out = (size_t)popcount(cond_mask & 3u) * (size_t)popcount(table_mask & 0x1ffu);
    // 1 B landcover read + n_out B written per pixel,
    // + the coarse soil window once, + the int32 index maps once.
    return (size_t)W * rows * (1 + n_out) + (size_t)(hsx > 0 ? hsx : 0) * (hsy > 0 ? hsy : 0) +
           4 * ((size_t)W + rows);
}

int gcn10_gpu_stream_copy(gcn10_gpu_ctx *ctx, const void *src, void *dst, size_t bytes, gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (bytes == 0)
        return GCN10_OK;
    if (!src || !dst || (bytes & 15u) || !aligned16(src) || !aligned16(dst) || bytes / 16 > 0x7fffffffull)
        return fail(GCN10_E_INVAL, "gcn10_gpu_stream_copy: needs 16-byte aligned pointers and size (< 32 GiB)");
    const u32x4 *in = static_cast<const u32x4 *>(src);
    u32x4 *out = static_cast<u32x4 *>(dst);
    uint32_t nvec = (uint32_t)(bytes / 16);
    uint32_t ntrips = (nvec + 2u * kThreads - 1u) / (2u * kThreads);
    const uint32_t grid = stream_grid(ctx, ntrips);
    hipStream_t s = as_stream(ctx, stream);
    void *args[] = { &in, &out, &nvec, &ntrips };
    HIP_TRY(launch_timed(ctx, reinterpret_cast<const void *>(stream_copy_kernel), grid, args, s));
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}

int gcn10_gpu_tune_single_raster(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                                 unsigned cond_mask, unsigned table_mask, uint8_t *arena, size_t arena_bytes,
                                 size_t step, uint8_t **best_out, float *best_ms, char *report, size_t report_cap,
                                 gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (!best_out || !arena || !esa || !cj)
        return fail(GCN10_E_INVAL, "gcn10_gpu_tune_single_raster: null pointer");
    if (popcount(cond_mask & 3u) != 1 || popcount(table_mask & 0x1ffu) != 1 || (cond_mask & ~3u) || (table_mask >> 9))
        return fail(GCN10_E_INVAL, "gcn10_gpu_tune_single_raster: exactly one condition and one table");
    if (W <= 0 || rows <= 0 || (uint64_t)W * (uint64_t)rows > 0x7fffffffull)
        return fail(GCN10_E_INVAL, "gcn10_gpu_tune_single_raster: bad shape %d x %d", W, rows);
    const size_t npix = (size_t)W * (size_t)rows;
    if (step == 0 || (step & 255u) || !aligned16(arena) || arena_bytes < npix)
        return fail(GCN10_E_INVAL, "gcn10_gpu_tune_single_raster: arena of %zu bytes / step %zu cannot hold a raster of %zu",
                    arena_bytes, step, npix);
    const int r = (cond_mask & 2u ? 9 : 0) + __builtin_ctz(table_mask);
    typedef gcn10_gpu_ctx::SingleShape Shape;
    // {set, xcd_slabs, grid_blocks_per_cu, ilp, prefetch}
    // XCD slabs only: a grid-stride sweep is 1-2 % faster at its best positions, but every XCD then pulls
    // every soil row through the fabric (FETCH_SIZE 1.18x the algorithmic bytes against 1.03x, profiles/r02)
    static const Shape shapes[] = { {true, 1, 8, 2, 1}, {true, 1, 16, 2, 1}, {true, 1, 8, 4, 0}, {true, 1, 16, 4, 0},
                                    {true, 1, 16, 1, 0}, {true, 1, 8, 2, 0}, {true, 1, 16, 2, 0}, {true, 1, 8, 1, 1} };
    const Shape saved = ctx->opt.single;
    hipStream_t s = as_stream(ctx, stream);
    constexpr int kRuns = 3;
    hipEvent_t e0[kRuns], e1[kRuns];
    for (int i = 0; i < kRuns; i++) {
        e0[i] = e1[i] = nullptr;
        if (hipEventCreate(&e0[i]) != hipSuccess || hipEventCreate(&e1[i]) != hipSuccess)
            return fail(GCN10_E_HIP, "gcn10_gpu_tune_single_raster: event creation failed");
    }
    float best = 1e30f, worst = 0.f;
    size_t best_pos = 0;
    Shape best_shape = shapes[0];
    int n_pos = 0;
    rc = GCN10_OK;
    for (size_t pos = 0; pos + npix <= arena_bytes && rc == GCN10_OK; pos += step, n_pos++) {
        uint8_t *out[GCN10_N_RASTERS] = { nullptr };
        out[r] = arena + pos;
        for (const Shape &sh : shapes) {
            ctx->opt.single = sh;
            rc = gcn10_gpu_cn_strip(ctx, esa, W, rows, cj, cond_mask, table_mask, out, stream);     // untimed
            for (int i = 0; i < kRuns && rc == GCN10_OK; i++) {
                ctx->time_start = e0[i];
                ctx->time_stop = e1[i];
                rc = gcn10_gpu_cn_strip(ctx, esa, W, rows, cj, cond_mask, table_mask, out, stream);
            }
            if (rc != GCN10_OK)
                break;
            if (hipStreamSynchronize(s) != hipSuccess) {
                rc = fail(GCN10_E_HIP, "gcn10_gpu_tune_single_raster: stream synchronisation failed");
                break;
            }
            float ms[kRuns];
            for (int i = 0; i < kRuns; i++)
                if (hipEventElapsedTime(&ms[i], e0[i], e1[i]) != hipSuccess)
                    ms[i] = 1e30f;
            // median of three
            const float lo = ms[0] < ms[1] ? ms[0] : ms[1], hi = ms[0] < ms[1] ? ms[1] : ms[0];
            const float med = ms[2] < lo ? lo : (ms[2] > hi ? hi : ms[2]);
            if (med < best) {
                best = med;
                best_pos = pos;
                best_shape = sh;
            }
            if (med > worst && med < 1e29f)
                worst = med;
        }
    }
    for (int i = 0; i < kRuns; i++) {
        (void)hipEventDestroy(e0[i]);
        (void)hipEventDestroy(e1[i]);
    }
    ctx->time_start = ctx->time_stop = nullptr;
    ctx->opt.single = saved;
    if (rc != GCN10_OK)
        return rc;
    ctx->opt.single = best_shape;
    *best_out = arena + best_pos;
    if (best_ms)
        *best_ms = best;
    if (report && report_cap)
        snprintf(report, report_cap,
                 "{\"positions\": %d, \"step_bytes\": %zu, \"shapes\": %zu, \"best_ms\": %.4f, \"worst_ms\": %.4f, "
                 "\"best_offset_bytes\": %zu, \"xcd_slabs\": %d, \"grid_blocks_per_cu\": %d, \"ilp1\": %d, \"prefetch\": %d}",
                 n_pos, step, sizeof shapes / sizeof shapes[0], best, worst, best_pos, best_shape.xcd_slabs,
                 best_shape.grid_blocks_per_cu, best_shape.ilp, best_shape.prefetch);
    return GCN10_OK;
}

}  // extern "C"
