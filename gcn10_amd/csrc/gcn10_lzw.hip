// gcn10_lzw.hip -- TIFF LZW encoding of CN raster tiles on the GPU (config key compress=lzw).
//
// What it is for: the reference's published runs wrote LZW GeoTIFFs (GTiff COMPRESS=LZW, TILED=YES), and so
// does every GIS user who reaches for GDAL's most common option.  This is the second codec behind the arena
// contract of gcn10_gpu_deflate_strip: every 256x256 tile of n_rasters CN strips held in HBM (edge tiles zero
// padded) becomes one complete TIFF 6.0 section 13 LZW stream, streams are packed into the caller's arena
// exactly as the DEFLATE tile encoders pack theirs (the placement pass B' of gcn10_arena_place.hip), and the
// sink, direct_io and the spill path of the host consume it unchanged.  The bytes are not libtiff's;
// decoded pixels are the parity target (tests decode every stream with a strict decoder of their own, with
// libtiff through PIL, and with the host reader, tiff_codec.c lzw_decode).
//
// Stream format: MSB-first codes of 9..12 bits (here 9 and 10), ClearCode 256, EndOfInformation 257, "early
// change" of the code width, EOI at the end, padded to a byte.  Every stream starts with ClearCode: libtiff
// takes a stream whose first byte is 0 and whose second has bit 0 set for old-style LSB-first LZW, which is
// what a tile whose first pixel is 0 would otherwise look like.
//
// Design.  LZW is serial within a stream, but the encoder may emit ClearCode anywhere, so a tile is cut into
// kSegs independently encoded segments of 64 rows (16 KiB), each with a fresh dictionary; their bit strings
// are concatenated (a segment ends with ClearCode, the last with EOI).  The dictionary is also cleared
// whenever the next code to assign would be 1023, so codes stay 9 or 10 bits wide and a dictionary holds at
// most 765 entries: a 1024-slot open-addressing hash of 32-bit slots (4 KiB, load <= 0.75) per segment.
// Measured on CN-like tiles against PIL's libtiff encoder (whole tile, dictionary up to 4093): 1.03x the bytes
// on patchy, 1.08x on noisy tiles; 16-row segments would cost 1.5x on patchy (LZW encoder).
//   pass L-A  one workgroup of one wave per tile; lanes 0..3 each encode one segment (the other lanes only
//             help clear the dictionaries): 16 KiB of LDS per tile = 10 tiles per CU (a 2048-slot hash, 32 KiB
//             per tile, 5 per CU, took 40.7 instead of 28.4 ms per 768-row 18-raster strip: the encoder is
//             bound by the latency of its dependent LDS probes, so resident lanes count).  Input is read straight
//             from the strip, 16 bytes per lane ahead of use; codes go to a workspace slot of the segment.
//             Dictionary slots carry a 4-bit generation, so a clear costs one increment (and a sweep of the
//             segment's 1024 slots every 15th clear).
//   pass B'   gcn10_arena_place.hip, as for the DEFLATE encoders: raster extents, 16-byte slots, cursor, 0xffffffff for
//             what does not fit the arena.
//   pass L-C  one workgroup per tile: every thread assembles whole 32-bit words of the stream from the
//             segments' bit strings (the segment bit offsets are a 4-entry prefix sum) and stores them into
//             the stream's slot.  The whole 16-byte slot is written: zero words behind the stream's last word,
//             nothing past the slot.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gcn10_deflate_internal.hpp"
#include "gcn10_gpu.h"
#include "gcn10_gpu_internal.hpp"

using gcn10::as_stream;
using gcn10::fail;
using gcn10::use_device;
using gcn10_deflate::kTile;
using gcn10_deflate::TileJob;

namespace {

constexpr int kSegs = 4;                            // segments per tile
constexpr int kSegRows = kTile / kSegs;             // 64 rows
constexpr int kSegBytes = kSegRows * kTile;         // 16 KiB
constexpr uint32_t kClear = 256, kEoi = 257, kFirst = 258;
constexpr uint32_t kCap = 1023;                     // ClearCode when the next code to assign reaches this
constexpr int kHashBits = 10, kSlots = 1 << kHashBits;
constexpr int kThreads = 64;

// Worst case of one segment (incompressible bytes): every code covers at least one byte, so at most kSegBytes
// data codes; a ClearCode follows every (kCap - kFirst) = 765 codes that assign an entry (the last code of a
// segment assigns none), so at most kSegBytes / 765 = 21 of them; one terminator (ClearCode or EOI); every
// code at most 10 bits.  Segment 0 also carries the stream's leading 9-bit ClearCode.
constexpr uint32_t kMaxClears = (uint32_t)kSegBytes / (kCap - kFirst);
constexpr uint32_t kSegMaxBits = 9u + ((uint32_t)kSegBytes + kMaxClears + 1u) * 10u;     // 164 069
constexpr uint32_t kSegWords = (kSegMaxBits + 31u) / 32u + 1u;      // + 1: pass L-C reads one word ahead
// the tile: 9 + 4 x 164 060 bits = 656 249 bits = 82 032 bytes (PIL/libtiff: 89 462 for i.i.d. bytes, 12-bit codes)
constexpr uint32_t kMaxStreamBits = 9u + (uint32_t)kSegs * (kSegMaxBits - 9u);
constexpr uint32_t kMaxStreamBytes = (kMaxStreamBits + 7u) / 8u;

struct LzwJob {
    const uint8_t *const *rasters;
    uint32_t *table;            // [n_tiles][2]: pass L-A writes { 0, bytes }, pass B' turns it into { offset, bytes }
    uint32_t *seg_words;        // [n_tiles][kSegs][kSegWords]: every segment's codes, MSB first (big-endian words)
    uint32_t *seg_bits;         // [n_tiles][kSegs]
    uint8_t *arena;
    uint32_t W, rows, across, down, n_tiles;
};

__device__ __forceinline__ uint32_t code_width(uint32_t next)
{
    return next < 512u ? 9u : 10u;      // next < kCap = 1023 always
}

// MSB-first bit writer into big-endian 32-bit words
struct BitOut {
    uint64_t acc = 0;
    uint32_t nacc = 0, words = 0;
    uint32_t *out;
    __device__ __forceinline__ void put(uint32_t code, uint32_t width)
    {
        acc = (acc << width) | code;
        nacc += width;
        if (nacc >= 32u) {
            nacc -= 32u;
            out[words++] = __builtin_bswap32((uint32_t)(acc >> nacc));
        }
    }
    __device__ __forceinline__ uint32_t finish()
    {
        if (nacc)
            out[words] = __builtin_bswap32((uint32_t)(acc << (32u - nacc)));
        return words * 32u + nacc;
    }
};

// 4 pixels of segment word i (row i / 64, columns 4 (i % 64) ..): zero outside the raster
__device__ __forceinline__ uint32_t load_word(const uint8_t *src, uint32_t W, uint32_t rows, uint32_t x0, uint32_t y0,
                                              uint32_t i)
{
    typedef uint32_t u32_u __attribute__((aligned(1)));
    const uint32_t y = y0 + (i >> 6), x = x0 + (i & 63u) * 4u;
    if (y >= rows || x >= W)
        return 0u;
    const uint8_t *p = src + (size_t)y * W + x;
    if (x + 4u <= W)
        return *reinterpret_cast<const u32_u *>(p);
    uint32_t v = 0;
    for (uint32_t b = 0; b < 4u && x + b < W; b++)
        v |= (uint32_t)p[b] << (8u * b);
    return v;
}

__global__ __launch_bounds__(kThreads) void lzw_encode_kernel(const LzwJob job)
{
    // slot: generation (4 bits, 0 = empty) | key = prefix code << 8 | byte (18 bits) | code (10 bits)
    __shared__ uint32_t dict[kSegs * kSlots];
    __shared__ uint32_t seg_bits[kSegs];
    const uint32_t tile = blockIdx.x;
    const uint32_t per_raster = job.across * job.down;
    const uint32_t r = tile / per_raster, pos = tile % per_raster;
    const uint32_t ty = pos / job.across, tx = pos % job.across;
    const uint32_t t = threadIdx.x;

    for (uint32_t i = t; i < (uint32_t)(kSegs * kSlots); i += kThreads)
        dict[i] = 0u;
    __syncthreads();
    if (t < (uint32_t)kSegs) {
        const uint8_t *src = job.rasters[r];
        const uint32_t x0 = tx * kTile, y0 = ty * kTile + t * kSegRows;
        uint32_t *tab = dict + t * kSlots;
        BitOut bo;
        bo.out = job.seg_words + ((size_t)tile * kSegs + t) * kSegWords;
        if (t == 0)
            bo.put(kClear, 9u);
        uint32_t gen = 1, next = kFirst, w = 0xffffffffu;
        uint64_t cur_lo, cur_hi;            // 16 pixels being encoded, the next 16 in flight
        {
            cur_lo = (uint64_t)load_word(src, job.W, job.rows, x0, y0, 0) |
                     (uint64_t)load_word(src, job.W, job.rows, x0, y0, 1) << 32;
            cur_hi = (uint64_t)load_word(src, job.W, job.rows, x0, y0, 2) |
                     (uint64_t)load_word(src, job.W, job.rows, x0, y0, 3) << 32;
        }
        for (uint32_t q = 0; q < (uint32_t)kSegBytes / 16u; q++) {
            uint64_t nxt_lo = 0, nxt_hi = 0;
            if (q + 1u < (uint32_t)kSegBytes / 16u) {
                const uint32_t i = (q + 1u) * 4u;
                nxt_lo = (uint64_t)load_word(src, job.W, job.rows, x0, y0, i) |
                         (uint64_t)load_word(src, job.W, job.rows, x0, y0, i + 1u) << 32;
                nxt_hi = (uint64_t)load_word(src, job.W, job.rows, x0, y0, i + 2u) |
                         (uint64_t)load_word(src, job.W, job.rows, x0, y0, i + 3u) << 32;
            }
            for (uint32_t j = 0; j < 16u; j++) {
                const uint32_t k = (uint32_t)((j < 8u ? cur_lo >> (8u * j) : cur_hi >> (8u * (j - 8u))) & 0xffu);
                if (w == 0xffffffffu) {
                    w = k;
                    continue;
                }
                const uint32_t key = (w << 8) | k;
                uint32_t h = (key * 0x9E3779B1u) >> (32 - kHashBits), found = 0xffffffffu;
                for (;;) {
                    const uint32_t v = tab[h];
                    if ((v >> 28) != gen)
                        break;
                    if (((v >> 10) & 0x3ffffu) == key) {
                        found = v & 0x3ffu;
                        break;
                    }
                    h = (h + 1u) & (uint32_t)(kSlots - 1);
                }
                if (found != 0xffffffffu) {
                    w = found;
                    continue;
                }
                bo.put(w, code_width(next));
                tab[h] = gen << 28 | key << 10 | next;
                if (++next == kCap) {
                    bo.put(kClear, code_width(next));
                    next = kFirst;
                    if (++gen == 16u) {         // generations used up: sweep this segment's slots
                        for (uint32_t s = 0; s < (uint32_t)kSlots; s++)
                            tab[s] = 0u;
                        gen = 1;
                    }
                }
                w = k;
            }
            cur_lo = nxt_lo;
            cur_hi = nxt_hi;
        }
        bo.put(w, code_width(next));
        // the decoder assigns an entry for that last code: the terminator is read one step later
        bo.put(t + 1u == (uint32_t)kSegs ? kEoi : kClear, code_width(next + 1u));
        const uint32_t bits = bo.finish();
        seg_bits[t] = bits;
        job.seg_bits[(size_t)tile * kSegs + t] = bits;
    }
    __syncthreads();
    if (t == 0) {
        uint32_t total = 0;
        for (int s = 0; s < kSegs; s++)
            total += seg_bits[s];
        job.table[(size_t)tile * 2] = 0u;
        job.table[(size_t)tile * 2 + 1] = (total + 7u) / 8u;
    }
}

// n <= 32 bits of a segment's bit string from bit `pos` (the word after the last written one is readable)
__device__ __forceinline__ uint32_t seg_get(const uint32_t *words, uint32_t pos, uint32_t n)
{
    const uint32_t i = pos >> 5, sh = pos & 31u;
    const uint64_t v = (uint64_t)__builtin_bswap32(words[i]) << 32 | __builtin_bswap32(words[i + 1u]);
    return (uint32_t)((v << sh) >> (64u - n));
}

__global__ __launch_bounds__(256) void lzw_pack_kernel(const LzwJob job)
{
    const uint32_t tile = blockIdx.x;
    const uint32_t off = job.table[(size_t)tile * 2], bytes = job.table[(size_t)tile * 2 + 1];
    if (off == 0xffffffffu)
        return;                             // did not fit the arena
    uint32_t base[kSegs + 1];
    base[0] = 0;
#pragma unroll
    for (int s = 0; s < kSegs; s++)
        base[s + 1] = base[s] + job.seg_bits[(size_t)tile * kSegs + s];
    const uint32_t *segw = job.seg_words + (size_t)tile * kSegs * kSegWords;
    uint32_t *dst = reinterpret_cast<uint32_t *>(job.arena + off);     // 16-byte aligned slot
    // the whole 16-byte slot: the words behind the stream's last one take bits of no segment and are stored as
    // zeros (the slot's tail goes into the raster's extent and from there into the file)
    const uint32_t n_words = (bytes + 15u) / 16u * 4u;
    for (uint32_t j = threadIdx.x; j < n_words; j += 256u) {
        const uint32_t p0 = j * 32u, p1 = p0 + 32u;
        uint32_t v = 0;
#pragma unroll
        for (int s = 0; s < kSegs; s++) {
            const uint32_t a = p0 > base[s] ? p0 : base[s], b = p1 < base[s + 1] ? p1 : base[s + 1];
            if (a < b)
                v |= seg_get(segw + (size_t)s * kSegWords, a - base[s], b - a) << (p1 - b);
        }
        dst[j] = __builtin_bswap32(v);
    }
}

}  // namespace

extern "C" {

size_t gcn10_gpu_lzw_arena_bound(int W, int rows, int n_rasters)
{
    return gcn10::arena_bound(W, rows, n_rasters, kMaxStreamBytes);
}

int gcn10_gpu_lzw_strip(gcn10_gpu_ctx *ctx, const uint8_t *const *rasters_dev, int n_rasters, int W, int rows,
                        uint8_t *arena_dev, size_t arena_cap, uint32_t *table_dev, unsigned long long *cursor_dev,
                        gcn10_stream_t stream)
{
    const char *const who = "gcn10_gpu_lzw_strip";
    int rc = use_device(ctx);
    if (rc)
        return rc;
    TileJob pj;                 // the strip's tile grid and where pass B' places: pass L-A leaves { 0, bytes } in the table
    rc = gcn10::tile_job_setup(who, W, rows, n_rasters, arena_dev, arena_cap, table_dev, cursor_dev, &pj);
    if (rc || pj.n_tiles == 0)
        return rc;              // refused, or an empty strip
    if (!rasters_dev)
        return fail(GCN10_E_INVAL, "%s: null pointer", who);
    LzwJob lj;
    lj.rasters = rasters_dev;
    lj.table = table_dev;
    lj.arena = arena_dev;
    lj.W = pj.W;
    lj.rows = pj.rows;
    lj.across = pj.across;
    lj.down = pj.down;
    lj.n_tiles = pj.n_tiles;

    const size_t need = (size_t)lj.n_tiles * kSegs * (kSegWords + 1u) * 4u;
    rc = gcn10::grow_workspace(&ctx->ws.lzw, &ctx->ws.lzw_cap, need);
    if (rc)
        return rc;
    lj.seg_words = reinterpret_cast<uint32_t *>(ctx->ws.lzw);
    lj.seg_bits = lj.seg_words + (size_t)lj.n_tiles * kSegs * kSegWords;

    hipStream_t s = as_stream(ctx, stream);
    HIP_TRY(hipMemsetAsync(cursor_dev, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(lzw_encode_kernel, dim3(lj.n_tiles), dim3(kThreads), 0, s, lj);
    HIP_TRY(hipGetLastError());
    rc = gcn10::launch_arena_place(ctx, pj, s);
    if (rc)
        return rc;
    hipLaunchKernelGGL(lzw_pack_kernel, dim3(lj.n_tiles), dim3(256), 0, s, lj);
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}

}  // extern "C"
