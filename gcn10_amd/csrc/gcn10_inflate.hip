// gcn10_inflate.hip -- zlib/DEFLATE decoding of landcover tiles on the GPU: the two kernels and the entry point.
//
// What it replaces: GDALRasterIO inside load_raster() (src/raster.c:167-176) inflates the ESA WorldCover tiles on the
// host before the pixel loop sees a byte; the VRT's sources are 36000x36000 DEFLATE GeoTIFFs with 1024x1024 internal
// tiles (landcover/esa_worldcover_2021.vrt:266-270), 1.3 GB decoded per block.  Here the *compressed* tiles cross PCIe
// (a few % of the raw bytes) and are decoded in HBM: a DEFLATE stream is serial, a block's ~1300 tiles are not, so one
// workgroup decodes one tile and a launch decodes them all.
//
// inflate_kernel: one workgroup of two wavefronts per stream (RFC 1950 wrapper, RFC 1951 stored / fixed / dynamic
// blocks).  The DECODER wave turns bits into tokens (literals, match, stored run), the COPIER wave carries tokens out;
// they swap halves of a 2 x kBatch-token ring at a barrier, so the bit decode never waits for a copy.
//   decoder  inside a block its lanes decode speculatively -- lane k the token that would start at bit P + k -- and a
//            scalar walk follows the real chain through them, which shrinks the serial part of the decode to a
//            v_readlane and a few scalar instructions per token (gcn10_inflate_decode.hpp; the bit reader and the
//            code tables it decodes with: gcn10_inflate_tables.hpp)
//   ring     the last kWindow = 8 KiB of output live in LDS, where reads after writes are ordered; a match whose
//            source has left the ring reads it back from HBM.  The copier sends every finished kFlush = 4 KiB to HBM,
//            16 bytes per lane, and takes a batch in sub-batches of at most kSubCap = 2 KiB, so that what is not
//            flushed yet, one sub-batch and the longest match fit the ring (gcn10_inflate_copy.hpp)
//   output   a tile whose whole chunk is wanted, a power of two wide, its rows on 16-byte boundaries of the destination
//            (tile_in_place: 94 % of a block's tiles, all but its last row and column) is flushed straight into the
//            raster's rows.  Every other tile decodes into its own linear slot
// untile_kernel copies the wanted window of every tile that was not decoded in place into the row-major landcover
// block: slot tiles, LZW tiles (lzw_decode_kernel's slots) and raw tiles (read where they lie among the staged bytes),
// summing TIFF Predictor 2 rows back on the way.  gcn10_inflate_internal.hpp has the contract of a tile for all three.
// Malformed streams end with a status code, never with a wild access or an endless loop (every trip of every loop
// consumes input bits, and input is bounded).
// How the ring came to 8 KiB and the copier to its five stages, with the measurements: DESIGN.md "Round 3" and the
// files of profiles/r03/ it names (inflate_window_*.txt, decoder_*_ab.txt, decoder_cycle_counters.txt).
//
// The three headers are pieces of this one translation unit, included inside its anonymous namespace: the decoder is
// one kernel, and TileIn is a parameter type of both kernels, so its namespace is part of their symbols.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "gcn10_gpu.h"
#include "gcn10_gpu_internal.hpp"
#include "gcn10_inflate_internal.hpp"
#include "gcn10_wave.hpp"

using gcn10::as_stream;
using gcn10::fail;
using gcn10::inflate_window_ok;
using gcn10::u32x4;
using gcn10::uniform;
using gcn10::use_device;
using gcn10::wave_scan;
using gcn10::wave_total;

namespace {

constexpr int kWindow = 8192;           // the LDS ring: output position p at window[p & kWindowMask]
constexpr int kWindowMask = kWindow - 1;
constexpr int kFlush = kWindow / 2;     // the copier sends the ring to HBM in units of this
constexpr uint32_t kSubCap = kWindow / 4;       // most bytes of a sub-batch of the copier, and of one stored-run token
constexpr uint32_t kShortMatch = 64;    // stage B takes matches up to this length (sixteen dword steps + up to three bytes)
constexpr int kBatch = 64;              // token words per hand-over from the decoder to the copier
constexpr int kCand = 4;                // candidate start bits per lane: a window of 64 * kCand bits
constexpr int kLitRoot = 10;
constexpr int kDistRoot = 9;
// copy_match: a sub-batch starts with fewer than kFlush bytes pending and ends at most kSubCap further, so a match
// source that the sub-batch's writes have overwritten in the ring has been flushed whole
static_assert(kFlush + (int)kSubCap + 258 <= kWindow && (kWindow & (kWindow - 1)) == 0 && kWindow >= 4096,
              "pending bytes, a sub-batch and the longest match fit the ring; its size is a power of two");

constexpr uint32_t kOk = 0;             // status of a sound stream; the others are GCN10_INFLATE_E_* (gcn10_gpu.h)

#include "gcn10_inflate_tables.hpp"

struct Shared {
    uint8_t window[kWindow];
    uint32_t lit_tab[1 << kLitRoot];        // decoded entries (gcn10_inflate_tables.hpp), 0 = longer code or none
    uint32_t dist_tab[1 << kDistRoot];
    uint16_t lit_sorted[288];
    uint16_t dist_sorted[32];
    uint8_t lens[320];
    Code lit, dist;
    // decoder wave -> copier wave: two batches of tokens (gcn10_inflate_decode.hpp), one being filled while the
    // other is carried out
    uint32_t ring[2][kBatch];
    uint32_t count[2];
    uint32_t stop;              // the trip after which both waves leave the loop
    uint32_t err;
};
static_assert(sizeof(Shared) <= 16 * 1024,
              "five decoder workgroups (a block's 1 296 streams) and a 77 KB encoder workgroup share a CU's 160 KiB of LDS");

struct TileIn {             // = gcn10_inflate_tile
    unsigned long long in_off;
    uint32_t in_len, out_len;
    uint32_t chunk_w, src_x, src_y, copy_w, copy_h, flags;       // GCN10_TILE_*
    unsigned long long dst_off;
};
static_assert(sizeof(TileIn) == sizeof(gcn10_inflate_tile), "TileIn mirrors the ABI struct");

#include "gcn10_inflate_decode.hpp"

#include "gcn10_inflate_copy.hpp"

// A tile inflate_kernel decodes straight into the destination raster (and untile_kernel leaves alone): see Output.
__device__ __forceinline__ bool tile_in_place(const TileIn &t, uint32_t slot_bytes, const uint8_t *dst, unsigned long long dst_stride)
{
    const uint32_t w = t.chunk_w;
    return !(t.flags & (GCN10_TILE_RAW | GCN10_TILE_PREDICTOR2 | GCN10_TILE_LZW)) && w >= 16u && (w & (w - 1u)) == 0u && t.src_x == 0u &&
           t.src_y == 0u && t.copy_w == w && t.copy_h > 0u && (unsigned long long)t.copy_h * w == t.out_len &&
           t.out_len <= slot_bytes && ((reinterpret_cast<uintptr_t>(dst) | t.dst_off | dst_stride) & 15u) == 0u;
}

// One workgroup of two wavefronts per stream: wave 0 decodes bits into tokens, wave 1 carries
// the tokens out; they swap halves of a small token ring at a barrier every kBatch tokens.
__global__ __launch_bounds__(128) void inflate_kernel(const uint8_t *comp, const TileIn *tiles, uint32_t n_tiles,
                                                      uint8_t *scratch, uint32_t slot_bytes, uint32_t *status,
                                                      uint8_t *dst, unsigned long long dst_stride)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    Shared &sh = *reinterpret_cast<Shared *>(smem);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t tile = blockIdx.x;
    if (tile >= n_tiles)
        return;
    const TileIn tin = tiles[tile];
    if (tin.flags & GCN10_TILE_LZW)
        return;                                 // lzw_decode_kernel's (gcn10_lzw_decode.hip)
    if (tin.flags & GCN10_TILE_RAW) {
        // not a zlib stream: the chunk's bytes lie in `comp` as they are; untile_kernel copies the window
        if (threadIdx.x == 0)
            status[tile] = tin.in_len >= tin.out_len &&
                                   inflate_window_ok(tin.out_len, tin.chunk_w, tin.src_x, tin.src_y, tin.copy_w, tin.copy_h,
                                             0xffffffffu)
                               ? 0u
                               : (uint32_t)GCN10_INFLATE_E_WINDOW;
        return;
    }

    Decoder d;
    d.r.in = reinterpret_cast<const uint32_t *>(comp + tin.in_off);
    d.r.n_dwords = (tin.in_len + 3u) / 4u;
    d.r.lane = lane;
    d.in_len = tin.in_len;
    d.state = kNeedHeader;
    d.P = 0;
    d.pos = 0;
    d.limit = tin.out_len < slot_bytes ? tin.out_len : slot_bytes;
    d.stored_left = d.stored_at = 0;
    d.err = kOk;
    d.last = false;
    Output o;
    o.out = scratch + (size_t)tile * slot_bytes;
    o.wshift = o.wmask = 0;
    o.stride = 0;
    if (tile_in_place(tin, slot_bytes, dst, dst_stride)) {
        o.out = dst + tin.dst_off;
        o.wshift = 31u - (uint32_t)__builtin_clz(tin.chunk_w);
        o.wmask = tin.chunk_w - 1u;
        o.stride = dst_stride;
    }
    o.limit = d.limit;
    o.pos = 0;
    o.flushed = 0;

    if (wave == 0) {
        reader_seek(d.r, 0);
        refill(d.r);
        const uint32_t cmf = take_bits(d.r, 8), flg = take_bits(d.r, 8);
        if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || (flg & 0x20u) || ((cmf << 8 | flg) % 31u) != 0u) {
            d.err = GCN10_INFLATE_E_HEADER;         // not a zlib stream (CM != 8, FDICT set, bad check bits)
            d.state = kDone;
        }
        if (lane == 0) {
            sh.stop = 0xffffffffu;
            sh.err = kOk;
            sh.count[0] = sh.count[1] = 0;
        }
    }
    __syncthreads();
    bool announced = false;
    uint32_t c_err = 0;
    for (uint32_t it = 0;; it++) {
        const uint32_t cur = it & 1u;
        if (wave == 0) {
            if (!announced) {
                const uint32_t n = decode_batch(sh, d, sh.ring[cur], lane);
                if (lane == 0)
                    sh.count[cur] = n;
                if (d.state == (uint32_t)kDone) {
                    if (!d.err && reader_byte_pos(d.r) > d.in_len + 4u)
                        d.err = GCN10_INFLATE_E_INPUT;      // ran past the end of the compressed bytes
                    if (lane == 0) {
                        sh.stop = it + 1u;          // the copier still has this batch to carry out
                        sh.err = d.err;
                    }
                    announced = true;
                }
            }
        }
        else if (it > 0 && c_err == 0) {
            c_err = copy_batch(sh, o, sh.ring[cur ^ 1u], uniform(sh.count[cur ^ 1u]), comp + tin.in_off, lane);
        }
        __syncthreads();
        if (it >= uniform(sh.stop))
            break;
    }
    if (wave == 0)
        return;
    uint32_t err = c_err ? c_err : uniform(sh.err);
    if (!err && !inflate_window_ok(tin.out_len, tin.chunk_w, tin.src_x, tin.src_y, tin.copy_w, tin.copy_h, slot_bytes))
        err = GCN10_INFLATE_E_WINDOW;

    // what is still in the window, then zeros up to the tile's size (as a short stream reads on the host)
    {
        const uint32_t end = o.pos < o.limit ? o.pos : o.limit;
        for (uint32_t i = o.flushed + (uint32_t)lane; i < end; i += 64)
            *out_at(o, i) = sh.window[i & kWindowMask];
        for (uint32_t i = end + (uint32_t)lane; i < tin.out_len && i < slot_bytes; i += 64)
            *out_at(o, i) = 0;
    }
    if (lane == 0)
        status[tile] = err;
}

// The wanted window of every decoded tile -> the row-major landcover block.  A raw tile
// (GCN10_TILE_RAW: TIFF Compression 1) is read where it lies among the staged bytes; a tile
// written with TIFF Predictor 2 (horizontal differencing, per chunk row) is summed back on the
// way: byte x of a row = sum of the stored bytes 0..x of that row, modulo 256 -- the inverse the
// host reader applies in tiff_codec.c, gcn10_tiff_decode_chunk().
__global__ __launch_bounds__(256) void untile_kernel(const TileIn *tiles, const uint8_t *scratch, uint32_t slot_bytes,
                                                     const uint8_t *comp, uint8_t *dst, unsigned long long dst_stride)
{
    typedef uint32_t u32_u __attribute__((aligned(1)));
    const TileIn tin = tiles[blockIdx.x];
    if ((tin.flags & (GCN10_TILE_RAW | GCN10_TILE_LZW)) == (GCN10_TILE_RAW | GCN10_TILE_LZW))
        return;                                 // no such tile: lzw_decode_kernel has set the status
    const bool raw = (tin.flags & GCN10_TILE_RAW) != 0;
    if (!inflate_window_ok(tin.out_len, tin.chunk_w, tin.src_x, tin.src_y, tin.copy_w, tin.copy_h, raw ? 0xffffffffu : slot_bytes) ||
        (raw && tin.in_len < tin.out_len))
        return;                                 // inflate_kernel has set the status
    if (tile_in_place(tin, slot_bytes, dst, dst_stride))
        return;                                 // inflate_kernel has written its rows where they belong
    const uint8_t *chunk = raw ? comp + tin.in_off : scratch + (size_t)blockIdx.x * slot_bytes;
    uint8_t *out = dst + tin.dst_off;
    const int lane = (int)(threadIdx.x & 63u);
    if (tin.flags & GCN10_TILE_PREDICTOR2) {
        // one wave per row, 1024 stored bytes per trip: 16 per lane summed in the lane, the lanes' totals
        // by a wave scan, the carry of the row's earlier trips on top
        const uint32_t end = tin.src_x + tin.copy_w;            // bytes of the row that matter
        for (uint32_t y = blockIdx.y * 4u + (threadIdx.x >> 6); y < tin.copy_h; y += gridDim.y * 4u) {
            const uint8_t *s = chunk + (size_t)(tin.src_y + y) * tin.chunk_w;
            uint8_t *d = out + (size_t)y * dst_stride;
            uint32_t carry = 0;
            for (uint32_t x0 = 0; x0 < end; x0 += 1024u) {
                const uint32_t x = x0 + (uint32_t)lane * 16u;
                uint8_t v[16];
                uint32_t acc = 0;
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    acc += x + (uint32_t)k < end ? s[x + (uint32_t)k] : 0u;
                    v[k] = (uint8_t)acc;
                }
                uint32_t incl = acc & 0xffu;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t up = __shfl_up(incl, off, 64);
                    if (lane >= off)
                        incl += up;
                }
                const uint32_t before = carry + incl - (acc & 0xffu);
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const uint32_t xx = x + (uint32_t)k;
                    if (xx >= tin.src_x && xx < end)
                        d[xx - tin.src_x] = (uint8_t)(v[k] + before);
                }
                carry = (carry + (uint32_t)__shfl(incl, 63, 64)) & 0xffu;
            }
        }
        return;
    }
    const uint8_t *src = chunk + (size_t)tin.src_y * tin.chunk_w + tin.src_x;
    // rows whose source and destination are 16-byte aligned (interior tiles of a window that starts on a multiple
    // of 16 pixels): 16 bytes per lane, a 1024-pixel row in one wave instruction each way
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(out) | tin.chunk_w | dst_stride | tin.copy_w) & 15u) == 0u) {
        const uint32_t w16 = tin.copy_w / 16u;
        for (uint32_t y = blockIdx.y * 4u + (threadIdx.x >> 6); y < tin.copy_h; y += gridDim.y * 4u) {
            const u32x4 *s = reinterpret_cast<const u32x4 *>(src + (size_t)y * tin.chunk_w);
            u32x4 *d = reinterpret_cast<u32x4 *>(out + (size_t)y * dst_stride);
            for (uint32_t i = threadIdx.x & 63u; i < w16; i += 64u)
                __builtin_nontemporal_store(__builtin_nontemporal_load(s + i), d + i);
        }
        return;
    }
    const uint32_t w4 = tin.copy_w / 4u;
    for (uint32_t y = blockIdx.y * 4u + (threadIdx.x >> 6); y < tin.copy_h; y += gridDim.y * 4u) {
        const uint8_t *s = src + (size_t)y * tin.chunk_w;
        uint8_t *d = out + (size_t)y * dst_stride;
        for (uint32_t i = threadIdx.x & 63u; i < w4; i += 64u)
            reinterpret_cast<u32_u *>(d)[i] = reinterpret_cast<const u32_u *>(s)[i];
        for (uint32_t i = w4 * 4u + (threadIdx.x & 63u); i < tin.copy_w; i += 64u)
            d[i] = s[i];
    }
}

}  // namespace

extern "C" {

int gcn10_gpu_inflate_tiles(gcn10_gpu_ctx *ctx, const uint8_t *comp_dev, const gcn10_inflate_tile *tiles_dev,
                            int n_tiles, uint32_t chunk_bytes, uint8_t *dst_dev, size_t dst_stride,
                            uint32_t *status_dev, gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (n_tiles < 0 || chunk_bytes == 0)
        return fail(GCN10_E_INVAL, "gcn10_gpu_inflate_tiles: bad shape (%d tiles of %u bytes)", n_tiles, chunk_bytes);
    if (n_tiles == 0)
        return GCN10_OK;
    if (!comp_dev || !tiles_dev || !dst_dev || !status_dev)
        return fail(GCN10_E_INVAL, "gcn10_gpu_inflate_tiles: null pointer");
    if ((reinterpret_cast<uintptr_t>(comp_dev) & 15u) != 0)
        return fail(GCN10_E_INVAL, "gcn10_gpu_inflate_tiles: compressed bytes must be 16-byte aligned");
    const uint32_t slot = (chunk_bytes + 255u) & ~255u;
    const size_t need = (size_t)slot * (size_t)n_tiles;
    rc = gcn10::grow_workspace(&ctx->ws.inflate, &ctx->ws.inflate_cap, need);
    if (rc)
        return rc;
    hipStream_t s = as_stream(ctx, stream);
    uint8_t *scratch = reinterpret_cast<uint8_t *>(ctx->ws.inflate);
    hipLaunchKernelGGL(inflate_kernel, dim3((uint32_t)n_tiles), dim3(128), sizeof(Shared), s, comp_dev,
                       reinterpret_cast<const TileIn *>(tiles_dev), (uint32_t)n_tiles, scratch, slot, status_dev,
                       dst_dev, (unsigned long long)dst_stride);
    // LZW tiles (GCN10_TILE_LZW) into their slots; every other tile leaves at once
    gcn10::launch_lzw_decode(comp_dev, tiles_dev, (uint32_t)n_tiles, scratch, slot, status_dev, s);
    hipLaunchKernelGGL(untile_kernel, dim3((uint32_t)n_tiles, 16), dim3(256), 0, s,
                       reinterpret_cast<const TileIn *>(tiles_dev), scratch, slot, comp_dev, dst_dev,
                       (unsigned long long)dst_stride);
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}

int gcn10_gpu_inflate_codecs(void)
{
    return (int)(GCN10_CODEC_DEFLATE | GCN10_CODEC_RAW | GCN10_CODEC_LZW);
}

}  // extern "C"
