// gcn10_deflate.hip -- zlib/DEFLATE encoding of CN raster tiles on the GPU: the per-raster encoder.
//
// What it replaces: GDAL's GTiff driver deflates every 256x256 block on the
// host inside save_raster()'s GDALRasterIO (the reference's src/raster.c:204-219,
// COMPRESS=DEFLATE, TILED=YES); the reference's paper names that as the cost
// that dominates a run (paper/paper.md:152-153).  With 18 rasters of 1.3 GB per
// block the raw rasters would also have to cross PCIe (23 GB per block).  Here
// the CN strips never leave HBM uncompressed: one workgroup per tile emits a
// complete zlib stream (RFC 1950 wrapper, one RFC 1951 dynamic-Huffman block,
// Adler-32), streams are packed into an arena, and only the arena is copied to
// the host, which appends the tiles to the GeoTIFFs.  Any inflate decodes them;
// the bytes differ from zlib's own output (file bytes are not a parity target,
// decoded pixels are: tests inflate every tile and compare).
//
// Encoder, five launches per strip (all tiles of all 18 rasters in each):
//   matches   only two distances are tried: 1 (run of the previous byte) and 256
//             (same column, row above) -- the two ways CN rasters repeat (10 m
//             landcover patches, 250 m soil cells); a match never crosses the end
//             of its row, so the 256 rows of a tile parse independently (greedy,
//             minimum length 3).  Candidates are found with byte-compare bit masks,
//             so literal stretches and run lengths cost a few bit operations
//   pass A    here: one workgroup per tile (thread t = row t): symbol statistics, Adler-32
//   pass B    gcn10_deflate_codes.hip: every tile's Huffman code, block header and stream size
//   pass B'   gcn10_arena_place.hip: one workgroup lays the streams out, one extent per raster
//   pass C    here, two launches (streams of at most kSmallStream bytes, two workgroups per CU;
//             the others): one workgroup per tile, rows re-parse, sum their bit lengths, a prefix
//             sum places them, rows OR their bits into an LDS image of the stream;
//             stored-block fallback when Huffman coding would exceed the raw size
// The fused encoder (gcn10_deflate_fused.hip) writes the same streams without the CN rasters.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "gcn10_deflate_internal.hpp"
#include "gcn10_gpu.h"
#include "gcn10_gpu_internal.hpp"

using gcn10::as_stream;
using gcn10::fail;
using gcn10::u32x4;
using gcn10::use_device;
using namespace gcn10_deflate;

namespace {

// ------------------------------------------------------------------------
// shared by passes A and C: the tile in LDS and the row parser
// ------------------------------------------------------------------------

// One wave reads one 256-byte tile row per step (coalesced); rows need not be
// dword aligned (W = 36001 blocks), gfx950 serves unaligned dword loads.  Pixels
// outside the raster are zero, as GDAL pads edge blocks.
__device__ __forceinline__ void load_tile(const TileJob &job, const uint8_t *src, uint32_t tx, uint32_t ty,
                                          uint8_t *tile, int t)
{
    typedef uint32_t u32_u __attribute__((aligned(1)));
    const uint32_t x = tx * kTile + (uint32_t)(t & 63) * 4u;
    const uint32_t y0 = ty * kTile + (uint32_t)(t >> 6);
    uint32_t *dst = reinterpret_cast<uint32_t *>(tile) + (t & 63);
    if ((tx + 1) * kTile <= job.W && (ty + 1) * kTile <= job.rows) {
        // interior tile: 64 independent loads per thread, all in flight at once
        const uint8_t *p = src + (size_t)y0 * job.W + x;
        const size_t step = (size_t)job.W * 4;
        uint32_t v[kTile / 4];
#pragma unroll
        for (int i = 0; i < kTile / 4; i++)
            v[i] = *reinterpret_cast<const u32_u *>(p + (size_t)i * step);
#pragma unroll
        for (int i = 0; i < kTile / 4; i++)
            dst[(i * 4 + (t >> 6)) * (kRowStride / 4)] = v[i];
        return;
    }
    for (int i = 0; i < kTile / 4; i++) {
        const int r = i * 4 + (t >> 6);
        const uint32_t y = ty * kTile + (uint32_t)r;
        uint32_t v = 0;
        if (y < job.rows && x < job.W) {
            const uint8_t *p = src + (size_t)y * job.W + x;
            if (x + 4u <= job.W) {
                v = *reinterpret_cast<const u32_u *>(p);
            }
            else {
                for (uint32_t k = 0; x + k < job.W; k++)
                    v |= (uint32_t)p[k] << (8 * k);
            }
        }
        dst[r * (kRowStride / 4)] = v;
    }
}


// What a row parse does with each token.
enum { kCount = 0, kMeasure = 1, kEmit = 2 };

struct CodeView {               // the code book as the parser sees it (LDS)
    const uint8_t *lit_len;
    const uint16_t *lit_code;
    uint8_t dist_len[2];
    uint16_t dist_code[2];
};

struct RowEmitter {
    uint32_t *out;
    uint32_t pos;
    unsigned long long acc;
    int nacc;
    __device__ __forceinline__ void put(uint32_t value, int nbits)
    {
        acc |= (unsigned long long)value << nacc;
        nacc += nbits;
        if (nacc >= 32) {
            const uint32_t lo = (uint32_t)acc;
            const uint32_t w = pos >> 5, sh = pos & 31;
            atomicOr(&out[w], lo << sh);
            if (sh)
                atomicOr(&out[w + 1], lo >> (32 - sh));
            acc >>= 32;
            nacc -= 32;
            pos += 32;
        }
    }
    __device__ __forceinline__ void finish()
    {
        if (nacc > 0) {
            const uint32_t lo = (uint32_t)acc & (0xffffffffu >> (32 - nacc));
            const uint32_t w = pos >> 5, sh = pos & 31;
            atomicOr(&out[w], lo << sh);
            if (sh && sh + nacc > 32)
                atomicOr(&out[w + 1], lo >> (32 - sh));
            pos += nacc;
            nacc = 0;
            acc = 0;
        }
    }
};

// Greedy parse of tile row t (matches of length >= 3 at distance 1 or 256, never
// crossing the row's end).  Literal stretches are skipped with the masks; only
// the literal bytes themselves are read from LDS.
template <int MODE>
__device__ __forceinline__ uint32_t parse_row(const uint8_t *tile, int t, const RowMasks &m,
                                              uint32_t *lit_hist, uint32_t *dist_hist,
                                              const CodeView *cv, RowEmitter *em)
{
    const uint8_t *row = tile + t * kRowStride;
    uint32_t bits = 0;
    int x = 0;

    while (x < kTile) {
        const int cand = next_candidate(m, x);
        // literals up to the next position where a match could start
        for (; x < cand; x++) {
            const int s = row[x];
            if (MODE == kCount)
                atomicAdd(&lit_hist[s], 1u);
            else if (MODE == kMeasure)
                bits += cv->lit_len[s];
            else
                em->put(cv->lit_code[s], cv->lit_len[s]);
        }
        if (x >= kTile)
            break;
        const int l1 = run_from(m.near_, x);
        const int l256 = run_from(m.far_, x);
        const bool far = l256 > l1;                 // tie: distance 1 (no extra bits)
        const int len = far ? l256 : l1;            // <= 256 - x by construction
        if (len >= 3) {
            const int lc = length_code(len);
            const int ls = 257 + lc;
            const int di = far ? 1 : 0;
            if (MODE == kCount) {
                atomicAdd(&lit_hist[ls], 1u);
                atomicAdd(&dist_hist[di], 1u);
            }
            else if (MODE == kMeasure) {
                bits += cv->lit_len[ls] + kLenExtra[lc] + cv->dist_len[di] + (far ? 6 : 0);
            }
            else {
                em->put(cv->lit_code[ls], cv->lit_len[ls]);
                if (kLenExtra[lc])
                    em->put((uint32_t)(len - kLenBase[lc]), kLenExtra[lc]);
                em->put(cv->dist_code[di], cv->dist_len[di]);
                if (far)
                    em->put(63u, 6);                // 256 - 193: distance code 15 has 6 extra bits
            }
            x += len;
        }
        else {
            const int s = row[x];
            if (MODE == kCount)
                atomicAdd(&lit_hist[s], 1u);
            else if (MODE == kMeasure)
                bits += cv->lit_len[s];
            else
                em->put(cv->lit_code[s], cv->lit_len[s]);
            x++;
        }
    }
    return bits;
}

// ------------------------------------------------------------------------
// pass A: symbol statistics + Adler-32, one workgroup per tile
// ------------------------------------------------------------------------
struct SharedA {
    uint8_t tile[kTile * kRowStride];
    uint32_t lit_hist[288];
    uint32_t dist_hist[2];
    uint32_t adler_a[kTile];
    uint32_t adler_b[kTile];
};

__global__ __launch_bounds__(kTile) void deflate_stats_kernel(const TileJob job)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    SharedA &sh = *reinterpret_cast<SharedA *>(smem);
    const int t = threadIdx.x;
    const uint32_t tiles = job.across * job.down;
    const uint32_t raster = blockIdx.x / tiles;
    const uint32_t tix = blockIdx.x - raster * tiles;
    const uint32_t ty = tix / job.across, tx = tix - ty * job.across;

    load_tile(job, job.rasters[raster], tx, ty, sh.tile, t);
    for (int i = t; i < 288; i += kTile)
        sh.lit_hist[i] = 0;
    if (t < 2)
        sh.dist_hist[t] = 0;
    __syncthreads();

    // Adler-32 partial sums of row t: A = sum x, B = sum (n - i) x_i over the row,
    // n = 65536, i = 256 t + k the byte's position in the tile
    {
        const uint32_t *row = reinterpret_cast<const uint32_t *>(sh.tile + t * kRowStride);
        uint32_t a = 0, b = 0;
#pragma unroll 8
        for (int j = 0; j < kTile / 4; j++) {
            const uint32_t v = row[j];
            const uint32_t b0 = v & 0xff, b1 = (v >> 8) & 0xff, b2 = (v >> 16) & 0xff, b3 = v >> 24;
            a += b0 + b1 + b2 + b3;
            b += (uint32_t)(kTile - 4 * j) * b0 + (uint32_t)(kTile - 4 * j - 1) * b1 +
                 (uint32_t)(kTile - 4 * j - 2) * b2 + (uint32_t)(kTile - 4 * j - 3) * b3;
        }
        sh.adler_a[t] = a;      // <= 256 * 255
        sh.adler_b[t] = (uint32_t)(((unsigned long long)b +
                                    (unsigned long long)(kTileBytes - kTile * (t + 1)) * a) % 65521ull);
    }

    RowMasks m;
    row_masks(sh.tile, t, m);
    parse_row<kCount>(sh.tile, t, m, sh.lit_hist, sh.dist_hist, nullptr, nullptr);
    // a tile of one value (ocean, no-data: most of the globe): every byte repeats its
    // predecessor.  Pass C then emits it without loading the tile again.
    const bool row_constant = (m.near_[0] | (t == 0 ? 1ull : 0ull)) == ~0ull && m.near_[1] == ~0ull &&
                              m.near_[2] == ~0ull && m.near_[3] == ~0ull;
    const bool tile_uniform = __syncthreads_and(row_constant) != 0;

    uint32_t *out = job.hist + (size_t)blockIdx.x * kHistWords;
    for (int i = t; i < 288; i += kTile)
        out[i] = i == 256 ? 1u : sh.lit_hist[i];       // 256 = end of block, once
    if (t < 2)
        out[288 + t] = sh.dist_hist[t];
    // tree reduction of the 256 partial sums (both stay below 2^32)
    for (int off = kTile / 2; off > 0; off >>= 1) {
        if (t < off) {
            sh.adler_a[t] += sh.adler_a[t + off];
            sh.adler_b[t] += sh.adler_b[t + off];
        }
        __syncthreads();
    }
    if (t == 0) {
        const uint32_t s1 = (1u + sh.adler_a[0]) % 65521u;
        const uint32_t s2 = (uint32_t)(((unsigned long long)kTileBytes + sh.adler_b[0]) % 65521ull);
        out[290] = (s2 << 16) | s1;
        out[291] = tile_uniform ? (1u | ((uint32_t)sh.tile[0] << 8)) : 0u;
    }
}

// ------------------------------------------------------------------------
// pass C: measure, place and emit; one workgroup per tile
// ------------------------------------------------------------------------
template <bool SMALL>
struct SharedC {
    static constexpr int kWords = SMALL ? kSmallStream / 4 + 16 : kOutWords;
    uint8_t tile[kTile * kRowStride];
    uint32_t out[kWords];
    uint8_t lit_len[288];
    uint16_t lit_code[288];
    uint32_t wave_sum[4];
};

// inclusive prefix sum over the 256 threads of the workgroup (4 waves of 64)
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t *wave_sum, int t)
{
    const int lane = t & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(v, off, 64);
        if (lane >= off)
            v += up;
    }

    if (lane == 63)
        wave_sum[t >> 6] = v;
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < (t >> 6); w++)
        base += wave_sum[w];
    return v + base;
}

// SMALL = true : streams of at most kSmallStream bytes, LDS for two workgroups per CU
// SMALL = false: the others (noisy tiles, stored fallback), one workgroup per CU
template <bool SMALL>
__global__ __launch_bounds__(kTile) void deflate_emit_kernel(const TileJob job)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    SharedC<SMALL> &sh = *reinterpret_cast<SharedC<SMALL> *>(smem);
    const int t = threadIdx.x;
    const Book *book = reinterpret_cast<const Book *>(job.books + (size_t)blockIdx.x * kBookBytes);
    const uint32_t stream_bytes = book->stream_bytes;
    if ((stream_bytes <= (uint32_t)kSmallStream) != SMALL)
        return;                                     // the other launch emits this tile
    const uint32_t slot = job.table[(size_t)blockIdx.x * 2];       // placed by deflate_place_kernel
    if (slot == 0xffffffffu)
        return;                                     // arena too small: the table says so
    const uint32_t tiles = job.across * job.down;
    const uint32_t raster = blockIdx.x / tiles;
    const uint32_t tix = blockIdx.x - raster * tiles;
    const uint32_t ty = tix / job.across, tx = tix - ty * job.across;
    const uint32_t header_bits = book->header_bits;
    const uint32_t adler = job.hist[(size_t)blockIdx.x * kHistWords + 290];
    const bool stored = stream_bytes == (uint32_t)kMaxStream;
    const uint32_t n_words = (stream_bytes + 3) / 4;
    const uint32_t uniform_word = job.hist[(size_t)blockIdx.x * kHistWords + 291];
    const bool uniform = (uniform_word & 1u) != 0 && !stored;     // one-value tile: no need for its bytes

    if (!uniform)
        load_tile(job, job.rasters[raster], tx, ty, sh.tile, t);
    // the output image: block header from pass B, zeros up to the end of the stream's 16-byte slot (whole vectors
    // are stored below: the slot's tail goes into the raster's extent and from there into the file)
    const uint32_t nvec = (stream_bytes + 15) / 16;
    static_assert(SharedC<true>::kWords >= (kSmallStream + 15) / 16 * 4 + 1 && SharedC<false>::kWords >= (kMaxStream + 15) / 16 * 4 + 1,
                  "the output image holds the whole slot and the word the emitters may touch behind the stream");
    for (uint32_t i = t; i < (4 * nvec > n_words + 1 ? 4 * nvec : n_words + 1); i += kTile)
        sh.out[i] = (i < 64 && !stored) ? book->header[i] : 0u;
    for (int i = t; i < 288; i += kTile) {
        sh.lit_len[i] = book->lit_len[i];
        sh.lit_code[i] = book->lit_code[i];
    }
    CodeView cv;
    cv.lit_len = sh.lit_len;
    cv.lit_code = sh.lit_code;
    cv.dist_len[0] = book->dist_len[0];
    cv.dist_len[1] = book->dist_len[1];
    cv.dist_code[0] = book->dist_code[0];
    cv.dist_code[1] = book->dist_code[1];
    __syncthreads();

    uint8_t *o = reinterpret_cast<uint8_t *>(sh.out);
    if (uniform) {
        // the greedy parse of a one-value tile, written out: row 0 = literal + match(255, 1),
        // every other row = match(256, 1); both lengths use length code 27 (227..257, 5 extra bits)
        const uint32_t v = (uniform_word >> 8) & 0xffu;
        const int ls = 257 + 27;
        const uint32_t match_bits = (uint32_t)sh.lit_len[ls] + 5u + cv.dist_len[0];
        const uint32_t row0_bits = (uint32_t)sh.lit_len[v] + match_bits;
        RowEmitter em{ sh.out, header_bits + (t == 0 ? 0u : row0_bits + (uint32_t)(t - 1) * match_bits), 0ull, 0 };
        if (t == 0)
            em.put(sh.lit_code[v], sh.lit_len[v]);
        em.put(sh.lit_code[ls], sh.lit_len[ls]);
        em.put((uint32_t)((t == 0 ? 255 : 256) - 227), 5);
        em.put(cv.dist_code[0], cv.dist_len[0]);
        if (t == kTile - 1)
            em.put(sh.lit_code[256], sh.lit_len[256]);      // end of block
        em.finish();
    }
    else if (!stored) {
        RowMasks m;
        row_masks(sh.tile, t, m);
        const uint32_t bits = parse_row<kMeasure>(sh.tile, t, m, nullptr, nullptr, &cv, nullptr);
        const uint32_t incl = block_scan(bits, sh.wave_sum, t);
        RowEmitter em{ sh.out, header_bits + incl - bits, 0ull, 0 };
        parse_row<kEmit>(sh.tile, t, m, nullptr, nullptr, &cv, &em);
        if (t == kTile - 1)
            em.put(sh.lit_code[256], sh.lit_len[256]);      // end of block
        em.finish();
    }
    else if (!SMALL) {
        // stored fallback: two blocks of 32768 bytes (LEN is 16 bit)
        if (t == 0) {
            o[0] = 0x78;
            o[1] = 0x01;
            for (int b = 0; b < 2; b++) {
                uint8_t *h = o + 2 + b * (5 + 32768);
                h[0] = (uint8_t)(b == 1);       // BFINAL, BTYPE = 00, padded to the byte
                h[1] = 0x00;
                h[2] = 0x80;                    // LEN = 32768
                h[3] = 0xff;
                h[4] = 0x7f;                    // NLEN
            }
        }
        // row t = bytes 256 t .. 256 t + 255 of the tile; block b holds rows 128 b ..
        uint8_t *dst = o + 2 + (t >> 7) * (5 + 32768) + 5 + (t & 127) * kTile;
        const uint8_t *row = sh.tile + t * kRowStride;
        for (int k = 0; k < kTile; k++)
            dst[k] = row[k];
    }
    __syncthreads();
    if (t == 0) {
        const uint32_t at = stream_bytes - 4;
        o[at] = (uint8_t)(adler >> 24);
        o[at + 1] = (uint8_t)(adler >> 16);
        o[at + 2] = (uint8_t)(adler >> 8);
        o[at + 3] = (uint8_t)adler;
    }
    __syncthreads();
    {
        u32x4 *dst = reinterpret_cast<u32x4 *>(job.arena + slot);
        const u32x4 *srcv = reinterpret_cast<const u32x4 *>(sh.out);
        for (uint32_t i = t; i < nvec; i += kTile)
            dst[i] = srcv[i];
    }
}

}  // namespace

extern "C" {

size_t gcn10_gpu_deflate_arena_bound(int W, int rows, int n_rasters)
{
    return gcn10::arena_bound(W, rows, n_rasters, kMaxStream);
}

int gcn10_gpu_deflate_strip(gcn10_gpu_ctx *ctx, const uint8_t *const *rasters_dev, int n_rasters, int W,
                            int rows, uint8_t *arena_dev, size_t arena_cap, uint32_t *table_dev,
                            unsigned long long *cursor_dev, gcn10_stream_t stream)
{
    const char *const who = "gcn10_gpu_deflate_strip";
    int rc = use_device(ctx);
    if (rc)
        return rc;
    TileJob job;
    rc = gcn10::tile_job_setup(who, W, rows, n_rasters, arena_dev, arena_cap, table_dev, cursor_dev, &job);
    if (rc || job.n_tiles == 0)
        return rc;                  // refused, or an empty strip
    if (!rasters_dev)
        return fail(GCN10_E_INVAL, "%s: null pointer", who);
    job.rasters = rasters_dev;

    // per-tile statistics and code books: workspace owned by the context
    const uint32_t nblocks = job.n_tiles;
    const size_t need = (size_t)nblocks * ((size_t)kHistWords * 4 + (size_t)kBookBytes);
    rc = gcn10::grow_workspace(&ctx->ws.deflate, &ctx->ws.deflate_cap, need);
    if (rc)
        return rc;
    job.hist = reinterpret_cast<uint32_t *>(ctx->ws.deflate);
    job.books = reinterpret_cast<uint8_t *>(ctx->ws.deflate) + (size_t)nblocks * kHistWords * 4;

    static_assert(sizeof(SharedC<false>) <= 160 * 1024, "tile + output image must fit the CU's 160 KiB of LDS");
    static_assert(sizeof(SharedC<true>) <= 80 * 1024, "two small-stream workgroups must fit one CU");
    static_assert(kBookBytes % 4 == 0, "code books are dword aligned");
    if (!ctx->deflate_ready) {
        HIP_TRY(gcn10::allow_dynamic_lds(deflate_stats_kernel, sizeof(SharedA)));
        HIP_TRY(gcn10::allow_dynamic_lds(deflate_emit_kernel<true>, sizeof(SharedC<true>)));
        HIP_TRY(gcn10::allow_dynamic_lds(deflate_emit_kernel<false>, sizeof(SharedC<false>)));
        ctx->deflate_ready = true;
    }
    hipStream_t s = as_stream(ctx, stream);
    HIP_TRY(hipMemsetAsync(cursor_dev, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(deflate_stats_kernel, dim3(nblocks), dim3(kTile), sizeof(SharedA), s, job);
    rc = gcn10::deflate_launch_codes(ctx, job, nblocks, s);
    if (rc)
        return rc;
    hipLaunchKernelGGL(deflate_emit_kernel<true>, dim3(nblocks), dim3(kTile), sizeof(SharedC<true>), s, job);
    hipLaunchKernelGGL(deflate_emit_kernel<false>, dim3(nblocks), dim3(kTile), sizeof(SharedC<false>), s, job);
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}
}  // extern "C"
