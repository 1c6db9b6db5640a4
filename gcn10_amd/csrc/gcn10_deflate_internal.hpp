// gcn10_deflate_internal.hpp -- shared by the three tile encoders of libgcn10_gpu.so and the passes they have in
// common:
//   gcn10_deflate.hip        one zlib stream per tile of a CN raster held in HBM (passes A and C)
//   gcn10_deflate_fused.hip  the 18 streams of a tile position straight from landcover + soil (passes F-A and F-C)
//   gcn10_lzw.hip            one TIFF LZW stream per tile of a CN raster held in HBM
//   gcn10_deflate_codes.hip  pass B, code construction, which both DEFLATE encoders use unchanged
//   gcn10_arena_place.hip    pass B', where every stream goes in the arena, and the arena / table / cursor contract
//                            of all three: the job setup and the arena bound
// Constants, the hand-over structures between the passes, the match-candidate bit masks of the DEFLATE passes, and
// the declarations of what the last two files give the encoders.
#ifndef GCN10_DEFLATE_INTERNAL_HPP
#define GCN10_DEFLATE_INTERNAL_HPP

#include <hip/hip_runtime.h>

#include <cstdint>

#include "gcn10_gpu.h"
#include "gcn10_gpu_internal.hpp"
#include "gcn10_wave.hpp"

namespace gcn10_deflate {

constexpr int kTile = 256;
constexpr int kRowStride = 260;                 // 65 dwords: rows start in different LDS banks
constexpr int kTileBytes = kTile * kTile;
constexpr int kOutWords = 16416;                // 65 664 B: stored fallback (65 552 B) fits
constexpr int kMaxStream = 2 + 2 * 5 + kTileBytes + 4;     // stored: header, 2 blocks, adler
constexpr int kSlotAlign = 16;
// streams up to this size are emitted by the two-workgroups-per-CU variant of pass C
constexpr int kSmallStream = 12800;
constexpr int kNumLit = 286;
constexpr int kNumDist = 30;

// length 3..258 -> length code 0..28 (symbol 257 + code), RFC 1951 3.2.5
static __device__ const uint8_t kLenBase[29] = { 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31,
                                          35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 0 /*258*/ };
static __device__ const uint8_t kLenExtra[29] = { 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2,
                                           3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0 };
// order in which code-length-code lengths are sent, RFC 1951 3.2.7
static __device__ const uint8_t kClOrder[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
// the fixed, complete code for the code-length alphabet: symbols 0-9,16,17,18 get 4 bits,
// 10-15 get 5 bits (13/16 + 6/32 = 1).  Canonical codes, already bit-reversed.
static __device__ const uint8_t kClLen[19] = { 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 5, 5, 5, 5, 5, 5, 4, 4, 4 };

__device__ __forceinline__ uint32_t bitrev(uint32_t code, int len)
{
    return __builtin_bitreverse32(code) >> (32 - len);
}

__device__ __forceinline__ int length_code(int len)
{
    // len in 3..258
    if (len == 258)
        return 28;
    if (len <= 10)
        return len - 3;
    const int l = len - 3;
    const int hb = 31 - __builtin_clz(l);       // floor(log2(l)), >= 3
    const int eb = hb - 2;                      // extra bits
    return 4 * eb + 4 + ((l >> eb) & 3);
}

// length_code() and the value of the code's extra bits (len - kLenBase[code]) without the table: for len > 10,
// len - 3 = (4 + q) << eb | extra with q = two bits, so the extra bits are the low eb bits of len - 3
__device__ __forceinline__ int length_code_extra(int len, uint32_t &extra)
{
    extra = 0;
    if (len == 258)
        return 28;
    if (len <= 10)
        return len - 3;
    const int l = len - 3;
    const int eb = 29 - __builtin_clz(l);
    extra = (uint32_t)l & ((1u << eb) - 1u);
    return 4 * eb + 4 + ((l >> eb) & 3);
}

struct TileJob {
    const uint8_t *const *rasters;      // device array of raster strip pointers
    uint8_t *arena;
    uint32_t *table;                    // [n_rasters][tiles][2] = offset, size
    uint32_t *sizes;                    // [n_rasters][tiles][2] = alias mark or 0, bytes: what pass B leaves for the placement
                                        // (the table itself when pass B' places; a workspace array when pass F-C does)
    uint32_t *chunk_tot;                // [n_rasters][n_chunks] or null: 16-byte-aligned stream bytes of each 64 positions of a raster
    uint32_t n_chunks;                  // (pass F-C places from these: fused encoder, wave-independent emit)
    unsigned long long *cursor;
    uint32_t *hist;                     // [n_tiles][kHistWords]   (pass A -> B)
    uint8_t *books;                     // [n_tiles][kBookBytes]   (pass B -> C)
    uint32_t W, rows, across, down, n_tiles;
    unsigned long long arena_cap;
};

// per-tile statistics written by pass A: 288 literal/length counts, 2 distance
// counts (codes 0 and 15), the tile's Adler-32
constexpr int kHistWords = 288 + 2 + 2;
// per-tile code book written by pass B
struct Book {
    uint8_t lit_len[288];
    uint16_t lit_code[288];
    uint8_t dist_len[2];        // distance codes 0 (distance 1) and 15 (distance 256)
    uint8_t pad[2];
    uint16_t dist_code[2];
    uint32_t header_bits;       // bit position after the block header (zlib header included)
    uint32_t stream_bytes;      // size of the finished zlib stream (kMaxStream: stored fallback)
    uint32_t slot;              // its offset in the arena, 0xffffffff if the arena is too small
    uint32_t header[64];        // the first header_bits bits of the stream
};
constexpr int kBookBytes = (int)sizeof(Book);
// hist[291] of a (raster, tile): bit 0 = one-value tile (per-raster encoder: value << 8), bit 31 = this
// raster's tile is byte for byte the tile of selected raster (hist[291] & 0xff) -- fused encoder
constexpr uint32_t kAliasFlag = 0x80000000u;
constexpr uint32_t kAliasSlot = 0xfffffffeu;    // Book::slot of an alias (0xffffffff: the arena is too small)

// ------------------------------------------------------------------------
// match candidates of a tile row as bit masks (passes A and C of both encoders)
// ------------------------------------------------------------------------

// 4 flag bits of a dword: bit k set iff byte k of d is zero
__device__ __forceinline__ uint32_t zero_bytes(uint32_t d)
{
    const uint32_t m = ~(((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d | 0x7f7f7f7fu);   // 0x80 per zero byte
    return (((m >> 7) * 0x00204081u) >> 21) & 0xfu;
}

// The two match candidates of every position of tile row t as bit masks:
// near bit x: byte x equals the previous byte of the stream (distance 1)
// far  bit x: byte x equals the byte above it (distance 256)
struct RowMasks {
    unsigned long long near_[4], far_[4];
};

__device__ __forceinline__ void row_masks(const uint8_t *tile, int t, RowMasks &m)
{
    const uint32_t *row = reinterpret_cast<const uint32_t *>(tile + t * kRowStride);
    const uint32_t *above = reinterpret_cast<const uint32_t *>(tile + (t - 1) * kRowStride);
    uint32_t prev = t > 0 ? above[63] : 0u;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        unsigned long long nm = 0, fm = 0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t r = row[q * 16 + j];
            const uint32_t shifted = (r << 8) | (prev >> 24);
            nm |= (unsigned long long)zero_bytes(r ^ shifted) << (4 * j);
            if (t > 0)
                fm |= (unsigned long long)zero_bytes(r ^ above[q * 16 + j]) << (4 * j);
            prev = r;
        }
        m.near_[q] = nm;
        m.far_[q] = fm;
    }
    if (t == 0)
        m.near_[0] &= ~1ull;        // the tile's first byte has no predecessor
}

__device__ __forceinline__ unsigned long long pick(const unsigned long long (&m)[4], int w)
{
    return w == 0 ? m[0] : w == 1 ? m[1] : w == 2 ? m[2] : m[3];
}

// number of consecutive set bits starting at bit x (0 <= x < 256)
__device__ __forceinline__ int run_from(const unsigned long long (&m)[4], int x)
{
    int len = 0;
    for (;;) {
        const int pos = x + len;
        if (pos >= kTile)
            return len;
        const int b = pos & 63;
        const unsigned long long inv = ~(pick(m, pos >> 6) >> b);
        const int n = inv ? __builtin_ctzll(inv) : 64;
        if (n < 64 - b)
            return len + n;
        len += 64 - b;
    }
}

// next position >= x where either mask has a set bit (256 if none)
__device__ __forceinline__ int next_candidate(const RowMasks &m, int x)
{
    for (int pos = x; pos < kTile;) {
        const int b = pos & 63;
        const unsigned long long v = (pick(m.near_, pos >> 6) | pick(m.far_, pos >> 6)) >> b;
        if (v)
            return pos + __builtin_ctzll(v);
        pos += 64 - b;
    }
    return kTile;
}

}  // namespace gcn10_deflate

namespace gcn10 {
using gcn10_deflate::TileJob;

// ---- gcn10_arena_place.hip: the arena / table / cursor contract of the three encoders ----
// The arguments every encoder entry point takes, checked, and the strip's tile grid worked out: `streams` is the
// number of streams per tile position (the rasters).  GCN10_E_INVAL ("<who>: ...") unless W > 0, rows >= 0 and
// 1 <= streams <= GCN10_N_RASTERS.  rows == 0 is an empty strip: GCN10_OK with job->n_tiles == 0 whatever the
// pointers are, and the caller returns without touching *cursor.  Otherwise GCN10_E_INVAL for a null arena, table or
// cursor, an arena that is not 16-byte aligned, an arena_cap that does not fit the 32-bit offsets of the table, and
// for 2^31 tiles or more.  On success *job holds arena, arena_cap, table, sizes (= table: pass B' places in the
// table itself), cursor, W, rows, across, down and n_tiles; everything else is zero, for the encoder to fill.
int tile_job_setup(const char *who, int W, int rows, int streams, uint8_t *arena, size_t arena_cap, uint32_t *table,
                   unsigned long long *cursor, TileJob *job);
// the arena that holds n_rasters strips of W x rows whatever their content: streams of at most max_stream bytes
size_t arena_bound(int W, int rows, int n_rasters, size_t max_stream);
// Pass B' (deflate_place_kernel): lays out the streams whose sizes lie in job.sizes (= job.table: { alias mark or 0,
// bytes } per stream), writes their offsets to job.table and the bytes used to *job.cursor.
int launch_arena_place(gcn10_gpu_ctx *ctx, const TileJob &job, hipStream_t s);

// ---- gcn10_deflate_codes.hip ----
// Pass B for `nblocks` (raster, tile) pairs whose statistics are in job.hist: code books to job.books,
// sizes to job.sizes; with `place`, pass B' behind it lays the streams out in the arena.
int deflate_launch_codes(gcn10_gpu_ctx *ctx, const TileJob &job, uint32_t nblocks, hipStream_t s, bool place = true);

// More than 64 KiB of dynamic LDS per workgroup has to be asked for, once per kernel and device: the launch function
// of the file that owns the kernel does, behind a flag of the context.
template <typename Kernel>
inline hipError_t allow_dynamic_lds(Kernel *kernel, size_t bytes)
{
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)bytes);
}

}  // namespace gcn10

#endif
