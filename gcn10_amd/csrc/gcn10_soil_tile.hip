// gcn10_soil_tile.hip -- the prepared soil tile: gcn10_gpu_prepare_tile, the code bytes made on demand, and the host
// preamble of every reader of the tile (gcn10::check_tile, bind_soil).
//
// Reference behaviour restated here (citations are paths of the reference):
//   src/cn.c:218-232   HSG nearest-neighbour upsample  -> x-expand + row pick
//   src/cn.c:88-111    modify_hysogs_data              -> soil-code byte (sD | sU<<4)
//
// Data layout in HBM (gcn10_gpu_ctx::Tile):
//   codes    [hsy][codes_stride] one byte per coarse soil cell holding both remapped
//                                soil groups, and cx[W'], the coarse column of every fine
//                                column (2.1 MB + 144 KB): what the strips of 16-byte aligned
//                                rows read, and the snapshot hx is made from
//   hx       [hsy][hx_stride]    the same codes expanded along x, one byte per fine
//                                column (52 MB for a 36000-wide block); made on demand
//                                for the kernels that read soil per pixel (soil_bytes)

#include <hip/hip_runtime.h>

#include <cstdint>

#include "gcn10_gpu.h"
#include "gcn10_device_util.hpp"
#include "gcn10_gpu_internal.hpp"
#include "gcn10_soil_readers.hpp"

using gcn10::aligned16;
using gcn10::as_stream;
using gcn10::fail;
using gcn10::kInvalidPlane;
using gcn10::kThreads;
using gcn10::load16_any;
using gcn10::soil_code;
using gcn10::SoilView;
using gcn10::u32x4;
using gcn10::use_device;

namespace {

// ------------------------------------------------------------------------
// The soil of a prepared tile (the x half of src/cn.c:218-232).  The fine soil code of column x in coarse row r is
// soil_code(coarse[r][ci[x]]).  gcn10_gpu_prepare_tile writes, into memory the context owns:
//   codes[r][c]  = soil_code(coarse[r][c]) for c < hsx, the "invalid" code for hsx <= c < codes_stride
//   cx[x]        = ci[x] clamped to the window, whatever its value; hsx (a column of padding codes) for the
//                  columns [W, hx_stride) right of the raster
// A 16-px column group g is COMPACT when its columns are a run of c_lo = cx[16g] followed by a run of
// c_hi = cx[16g + 15]: pixels [0, split) have the code of c_lo and the rest the code of c_hi.  At the usual ratio
// (25 fine columns per coarse cell) every group has that form, and a lane of a strip kernel of 16-byte aligned rows,
// which stays in one column group, makes {c_lo, c_hi, split} from cx once and loads two code bytes per trip.
// A group that has no such form (three cells under 16 columns, a map that is not monotone) stores this tile's
// generation number in *complex (no reset between tiles needed); the strip kernels compare that word with the
// generation they were launched for and go through codes and cx pixel by pixel for the whole tile when it matches.
// codes and cx are a snapshot: the code bytes of the tile (expand_code_bytes) are made from them on demand, and the
// caller's coarse and ci are not read after this kernel.
// ------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kThreads) void soil_tables_kernel(const uint8_t *coarse, uint32_t hsx, uint32_t hsy,
                                                               const int32_t *ci, uint32_t W, uint32_t hx_stride,
                                                               uint8_t *codes, uint32_t codes_stride,
                                                               uint32_t *cx_out, uint32_t *complex, uint32_t gen)
{
    const uint32_t pad = (uint32_t)(kInvalidPlane | (kInvalidPlane << 4));
    if (blockIdx.y >= 1u) {
        // ---- codes: one thread = 16 consecutive cells of one coarse row ----
        const uint32_t per_row = codes_stride / 16u;
        const uint32_t t = ((blockIdx.y - 1u) * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
        const uint32_t r = t / per_row;
        if (r >= hsy)
            return;
        const uint32_t c0 = (t - r * per_row) * 16u;
        const uint8_t *row = coarse + (size_t)r * hsx;
        u32x4 in = { 0u, 0u, 0u, 0u };
        if (c0 + 16u <= hsx) {
            in = load16_any(row + c0);
        }
        else {
#pragma unroll
            for (int q = 0; q < 16; q++)
                if (c0 + q < hsx)
                    in[q >> 2] |= (uint32_t)row[c0 + q] << (8 * (q & 3));
        }
        u32x4 o;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            uint32_t w = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t code = c0 + 4 * j + q < hsx ? soil_code((uint8_t)(in[j] >> (8 * q))) : pad;
                w |= code << (8 * q);
            }
            o[j] = w;
        }
        *reinterpret_cast<u32x4 *>(codes + (size_t)r * codes_stride + c0) = o;
        return;
    }
    // ---- column map and the complex-tile word: one thread = 16 consecutive fine columns ----
    const uint32_t x = (blockIdx.x * blockDim.x + threadIdx.x) * 16u;
    if (x >= hx_stride)
        return;
    uint32_t cx[16];
    if (VEC && x + 16u <= W) {
        const u32x4 *civ = reinterpret_cast<const u32x4 *>(ci + x);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const u32x4 c4 = civ[j];
#pragma unroll
            for (int q = 0; q < 4; q++)
                cx[4 * j + q] = c4[q] < hsx ? c4[q] : hsx - 1u;
        }
    }
    else {
#pragma unroll
        for (int q = 0; q < 16; q++) {
            // (an index of the raster is clamped exactly as in the vector path, whatever its value;
            // only columns past W get the padding mark)
            const uint32_t xx = x + q;
            const uint32_t c = xx < W ? (uint32_t)ci[xx] : 0u;
            cx[q] = xx < W ? (c < hsx ? c : hsx - 1u) : hsx;
        }
    }
    // compact form: a run of c_lo followed by a run of c_hi (also: padding only, right of the raster)
    const uint32_t c_lo = cx[0], c_hi = cx[15];
    uint32_t split = 0;
    bool compact = true;
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const bool lo = cx[q] == c_lo;
        compact = compact && (lo ? split == (uint32_t)q : cx[q] == c_hi);
        split += lo && split == (uint32_t)q ? 1u : 0u;
    }
#pragma unroll
    for (int j = 0; j < 4; j++)
        *reinterpret_cast<u32x4 *>(cx_out + x + 4 * j) =
            u32x4{ cx[4 * j], cx[4 * j + 1], cx[4 * j + 2], cx[4 * j + 3] };
    if (x < W && !compact && *reinterpret_cast<volatile uint32_t *>(complex) != gen)
        *reinterpret_cast<volatile uint32_t *>(complex) = gen;      // every writer stores the same value
}

// ------------------------------------------------------------------------
// The code bytes of the prepared tile, for the kernels that read soil per pixel (gcn10::soil_bytes launches it
// when the first of them asks): hx[r][x] = codes[r][cx[x]].
// ------------------------------------------------------------------------
// coarse rows per thread: 2: 20.0 us, 3: 17.3, 4: 16.5, 6: 17.6 for a 36000 x 1440 window
// (profiles/r02/prepare_tile_rows_per_thread.txt, measured when this loop was part of prepare_tile)
constexpr uint32_t kExpandRows = 4;

__global__ __launch_bounds__(kThreads) void expand_code_bytes(const uint8_t *codes, uint32_t codes_stride,
                                                              uint32_t hsy, const uint32_t *cx_in, uint8_t *hx,
                                                              uint32_t hx_stride)
{
    // one thread = 16 consecutive fine columns of kExpandRows coarse rows: the 16 column indices are
    // loaded once, then per row byte gathers that hit L1/L2 (a row of codes is ~1.4 KB) and one 16-byte store
    const uint32_t x = (blockIdx.x * blockDim.x + threadIdx.x) * 16u;
    const uint32_t r0 = blockIdx.y * kExpandRows;
    if (x >= hx_stride || r0 >= hsy)
        return;
    uint32_t cx[16];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const u32x4 c4 = *reinterpret_cast<const u32x4 *>(cx_in + x + 4 * j);
#pragma unroll
        for (int q = 0; q < 4; q++)
            cx[4 * j + q] = c4[q];
    }
    // at the usual ratio (25 fine columns per coarse cell) 16 consecutive columns see at most two coarse
    // cells, the first column's and the last one's: two byte loads and 16 selects instead of 16 byte
    // gathers (the kernel is bound by the number of load instructions, not by bytes)
    const uint32_t c_lo = cx[0], c_hi = cx[15];
    bool two = true;
#pragma unroll
    for (int q = 0; q < 16; q++)
        two = two && (cx[q] == c_lo || cx[q] == c_hi);
    const uint32_t r1 = r0 + kExpandRows < hsy ? r0 + kExpandRows : hsy;
    for (uint32_t r = r0; r < r1; r++) {
        const uint8_t *row = codes + (size_t)r * codes_stride;
        u32x4 o;
        if (two) {
            const uint32_t code_lo = row[c_lo], code_hi = row[c_hi];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint32_t w = 0;
#pragma unroll
                for (int q = 0; q < 4; q++)
                    w |= (cx[4 * j + q] == c_lo ? code_lo : code_hi) << (8 * q);
                o[j] = w;
            }
        }
        else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint32_t w = 0;
#pragma unroll
                for (int q = 0; q < 4; q++)
                    w |= (uint32_t)row[cx[4 * j + q]] << (8 * q);
                o[j] = w;
            }
        }
        __builtin_nontemporal_store(o, reinterpret_cast<u32x4 *>(hx + (size_t)r * hx_stride + x));
    }
}

}  // namespace

namespace gcn10 {

int soil_bytes(gcn10_gpu_ctx *ctx, hipStream_t stream, const uint8_t **hx)
{
    *hx = nullptr;
    int rc = check_tile(ctx, "soil_bytes");
    if (rc)
        return rc;
    if (!ctx->tile.hx_made) {
        // the header's rule is all this relies on: `stream` is ordered after the prepare_tile that wrote the tables
        dim3 grid((ctx->tile.hx_stride / 16 + kThreads - 1) / kThreads, (ctx->tile.hx_rows + kExpandRows - 1) / kExpandRows);
        hipLaunchKernelGGL(expand_code_bytes, grid, dim3(kThreads), 0, stream, ctx->tile.d_codes, ctx->tile.codes_stride,
                           ctx->tile.hx_rows, ctx->tile.d_cx, ctx->tile.d_hx, ctx->tile.hx_stride);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ctx->tile.hx_made_ev, stream));
        ctx->tile.hx_made = true;
    }
    else {
        // whatever the stream: a handle compared with the expanding stream's could be a new stream's by now
        HIP_TRY(hipStreamWaitEvent(stream, ctx->tile.hx_made_ev, 0));
    }
    *hx = ctx->tile.d_hx;
    return GCN10_OK;
}

int check_tile(gcn10_gpu_ctx *ctx, const char *who)
{
    if (!ctx->tile.d_hx || ctx->tile.hx_W == 0)
        return fail(GCN10_E_STATE, "%s: call gcn10_gpu_prepare_tile first", who);
    return GCN10_OK;
}

int bind_soil(gcn10_gpu_ctx *ctx, const char *who, int W, hipStream_t stream, const int32_t *cj, SoilView *view)
{
    int rc = check_tile(ctx, who);
    if (rc)
        return rc;
    if (W <= 0 || (uint32_t)W != ctx->tile.hx_W)
        return fail(GCN10_E_STATE, "%s: the prepared tile is %u wide: call gcn10_gpu_prepare_tile for W=%d first", who,
                    ctx->tile.hx_W, W);
    view->cj = cj;
    view->stride = ctx->tile.hx_stride;
    view->rows = ctx->tile.hx_rows;
    return soil_bytes(ctx, stream, &view->hx);      // made on first use
}

}  // namespace gcn10

extern "C" {

int gcn10_gpu_prepare_tile(gcn10_gpu_ctx *ctx, const uint8_t *coarse, int hsx, int hsy,
                           const int32_t *ci, int W, gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (hsx <= 0 || hsy <= 0 || W <= 0)
        return fail(GCN10_E_INVAL, "gcn10_gpu_prepare_tile: bad shape W=%d soil=%dx%d", W, hsx, hsy);
    if (!coarse || !ci)
        return fail(GCN10_E_INVAL, "gcn10_gpu_prepare_tile: null pointer");
    // rows padded to a multiple of 16 plus one extra group so that any 16-byte
    // read starting below W stays inside the row
    const uint32_t stride = (((uint32_t)W + 15u) & ~15u) + 16u;
    const size_t need_hx = ((size_t)stride * (size_t)hsy + 63) & ~(size_t)63;
    // behind the code bytes: cx, codes (a row of codes ends with at least one padding code, which is what cx names
    // for the columns right of the raster, and what lets a strip lane load the two bytes at c_lo)
    const uint32_t codes_stride = (((uint32_t)hsx + 1u) + 15u) & ~15u;
    const size_t off_cx = (need_hx + 15) & ~(size_t)15;
    const size_t off_codes = (off_cx + (size_t)stride * 4u + 15) & ~(size_t)15;
    const size_t need = off_codes + (size_t)codes_stride * (size_t)hsy;
    // growing the workspace is the one allocation on this path; it happens
    // once per run for equally sized blocks.
    // The byte part is allocated here although it is filled only on demand: a reader never allocates.
    // 16 bytes in front of row 0: the strip kernel's second soil load of a lane that
    // straddles a row end starts up to 15 bytes before a soil row.
    // (no prepared tile while the workspace may change hands: a failed growth leaves the context in that state)
    ctx->tile.d_hx = nullptr;
    ctx->tile.hx_W = 0;
    rc = gcn10::grow_workspace(&ctx->tile.d_hx_alloc, &ctx->tile.hx_capacity, 16 + need);
    if (rc)
        return rc;
    ctx->tile.d_hx = static_cast<uint8_t *>(ctx->tile.d_hx_alloc) + 16;
    ctx->tile.d_cx = reinterpret_cast<uint32_t *>(ctx->tile.d_hx + off_cx);
    ctx->tile.d_codes = ctx->tile.d_hx + off_codes;
    ctx->tile.codes_stride = codes_stride;
    if (++ctx->tile.soil_gen == 0u)
        ctx->tile.soil_gen = 1u;      // 0 is what the word holds before the first complex tile
    ctx->tile.hx_made = false;
    ctx->tile.hx_stride = stride;
    ctx->tile.hx_W = (uint32_t)W;
    ctx->tile.hx_rows = (uint32_t)hsy;
    hipStream_t s = as_stream(ctx, stream);
    const uint32_t group_blocks = (stride / 16u + kThreads - 1) / kThreads;
    const size_t code_threads = (size_t)(codes_stride / 16u) * (size_t)hsy;
    const uint32_t code_chunks = (uint32_t)((code_threads + (size_t)group_blocks * kThreads - 1) / ((size_t)group_blocks * kThreads));
    auto fn = aligned16(ci) ? soil_tables_kernel<true> : soil_tables_kernel<false>;
    hipLaunchKernelGGL(fn, dim3(group_blocks, 1u + code_chunks), dim3(kThreads), 0, s, coarse, (uint32_t)hsx,
                       (uint32_t)hsy, ci, (uint32_t)W, stride, ctx->tile.d_codes, codes_stride, ctx->tile.d_cx,
                       ctx->tile.d_soil_complex, ctx->tile.soil_gen);
    HIP_TRY(hipGetLastError());
    // a tile whose strips are certain to read the bytes gets them now, behind the tables on the same stream
    if (!ctx->opt.compact_soil || (W & 15)) {
        const uint8_t *hx;
        return gcn10::soil_bytes(ctx, s, &hx);
    }
    return GCN10_OK;
}

int gcn10_gpu_soil_words_state(gcn10_gpu_ctx *ctx, gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (!ctx->opt.compact_soil || !ctx->tile.d_hx || ctx->tile.hx_W == 0)
        return 0;
    uint32_t flag = 0;
    hipStream_t s = as_stream(ctx, stream);
    HIP_TRY(hipMemcpyAsync(&flag, ctx->tile.d_soil_complex, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return flag == ctx->tile.soil_gen ? 2 : 1;
}

}  // extern "C"
