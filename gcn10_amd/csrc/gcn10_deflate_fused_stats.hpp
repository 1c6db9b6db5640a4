// gcn10_deflate_fused_stats.hpp -- pass F-A of the fused tile encoder (included by gcn10_deflate_fused.hip alone):
// one workgroup per tile position builds the class tile, parses it once and leaves the position's token stream and
// every raster's statistics.  Two forms with the same outputs, bit for bit: one lane per 64-pixel segment of a row
// (fused_stats_seg_kernel, the default) and one lane per row (fused_stats_kernel, option fused_parse = 0, the
// cross-check).  launch_fused_stats picks the form.
#ifndef GCN10_DEFLATE_FUSED_STATS_HPP
#define GCN10_DEFLATE_FUSED_STATS_HPP

#include "gcn10_deflate_fused_internal.hpp"

namespace {

// Class ids of one tile position into LDS (row stride kRowStride).  `soil_row` holds the soil
// row cj[y] of the tile's 256 rows (LDS), so that the landcover and soil-code loads of a tile
// depend on nothing and go out 16 rows at a time.
__device__ __forceinline__ void load_class_tile(const FusedJob &job, uint32_t tx, uint32_t ty,
                                                const uint8_t *class_of_lds, const uint32_t *soil_row,
                                                uint8_t *tile, int t)
{
    typedef uint32_t u32_u __attribute__((aligned(1)));
    const uint32_t x = tx * kTile + (uint32_t)(t & 63) * 4u;
    uint32_t *dst = reinterpret_cast<uint32_t *>(tile) + (t & 63);
    if ((tx + 1) * kTile <= job.t.W && (ty + 1) * kTile <= job.t.rows) {
        // interior tile: no edge cases
        const uint8_t *pe = job.esa + ((size_t)ty * kTile + (uint32_t)(t >> 6)) * job.t.W + x;
        for (int b = 0; b < kTile / 4; b += 16) {
            uint32_t e4[16], c4[16];
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int r = (b + i) * 4 + (t >> 6);
                e4[i] = *reinterpret_cast<const u32_u *>(pe + (size_t)(b + i) * 4 * job.t.W);
                c4[i] = *reinterpret_cast<const u32_u *>(job.soil.at(soil_row[r], x));
            }
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int r = (b + i) * 4 + (t >> 6);
                uint32_t out = 0;
#pragma unroll
                for (uint32_t q = 0; q < 4; q++) {
                    const uint32_t lc = (e4[i] >> (8 * q)) & 0xffu;
                    const uint32_t cc = compact_code((c4[i] >> (8 * q)) & 0xffu);
                    out |= (uint32_t)class_of_lds[cc * 256u + lc] << (8 * q);
                }
                dst[r * (kRowStride / 4)] = out;
            }
        }
        return;
    }
#pragma unroll 4
    for (int i = 0; i < kTile / 4; i++) {
        const int r = i * 4 + (t >> 6);
        dst[r * (kRowStride / 4)] = class_pixels4(job, x, ty * kTile + (uint32_t)r, class_of_lds);
    }
}

__device__ __forceinline__ void set_bit(unsigned long long (&m)[4], int x)
{
    const unsigned long long b = 1ull << (x & 63);
    const int w = x >> 6;
    m[0] |= w == 0 ? b : 0ull;
    m[1] |= w == 1 ? b : 0ull;
    m[2] |= w == 2 ? b : 0ull;
    m[3] |= w == 3 ? b : 0ull;
}

// next position >= x with a set bit (256 if none)
__device__ __forceinline__ int next_set(const unsigned long long (&m)[4], int x)
{
    for (int pos = x; pos < kTile;) {
        const int b = pos & 63;
        const unsigned long long v = pick(m, pos >> 6) >> b;
        if (v)
            return pos + __builtin_ctzll(v);
        pos += 64 - b;
    }
    return kTile;
}

// The greedy parse of parse_row(), done once per tile position and kept: statistics are
// counted, and the row is rewritten IN PLACE as its token stream.  A literal stays the byte
// it was (a class id); a match of length len at x (it covers >= 3 bytes) becomes
//   row[x]   = length code (0..28) | 0x80 if its distance is 256
//   row[x+1] = value of the length's extra bits | number of extra bits << 5
//   row[x+2] = len - 3
// and bit x of `start` is set.  Every mask of the tile must have been computed before.
// Returns the number of tokens of the row.
__device__ __forceinline__ uint32_t tokenise_row(uint8_t *tile, int t, const RowMasks &m, uint32_t *lit_hist,
                                                 uint32_t *dist_hist, unsigned long long (&start)[4])
{
    uint8_t *row = tile + t * kRowStride;
    int x = 0;
    uint32_t n_tokens = 0;
    start[0] = start[1] = start[2] = start[3] = 0ull;
    while (x < kTile) {
        const int cand = next_candidate(m, x);
        n_tokens += (uint32_t)(cand - x);
        for (; x < cand; x++)
            atomicAdd(&lit_hist[row[x]], 1u);
        if (x >= kTile)
            break;
        n_tokens++;
        const int l1 = run_from(m.near_, x);
        const int l256 = run_from(m.far_, x);
        const bool far = l256 > l1;                 // tie: distance 1 (no extra bits)
        const int len = far ? l256 : l1;
        if (len >= 3) {
            const int lc = length_code(len);
            const int ne = (lc < 8 || lc == 28) ? 0 : (lc - 4) >> 2;
            atomicAdd(&lit_hist[257 + lc], 1u);
            atomicAdd(&dist_hist[far ? 1 : 0], 1u);
            row[x] = (uint8_t)(lc | (far ? 0x80 : 0));
            row[x + 1] = (uint8_t)((len - kLenBase[lc]) | (ne << 5));
            row[x + 2] = (uint8_t)(len - 3);
            set_bit(start, x);
            x += len;
        }
        else {
            atomicAdd(&lit_hist[row[x]], 1u);
            x++;
        }
    }
    return n_tokens;
}

__device__ __forceinline__ uint32_t wave_sum64(uint32_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_xor(v, off, 64);
    return v;
}

struct SharedFA {
    uint8_t tile[kTile * kRowStride];
    uint32_t soil_row[kTile];           // cj[y] of the tile's rows, clamped
    union {
        uint8_t class_of[gcn10::kClassCodes * 256];     // while the tile is built
        struct {
            uint32_t lit_hist[288];     // literals by class, match length symbols at 257..
            uint32_t dist_hist[2];
            uint32_t n_c[256], w_c[256];                // pixels per class, sum of their Adler weights
            uint32_t H[kGroup][256];                    // literal counts by VALUE, kGroup rasters at a time
            uint32_t s1[GCN10_N_RASTERS], s2[GCN10_N_RASTERS];
            uint32_t row_base[4];
            uint32_t sig[GCN10_N_RASTERS], cand[GCN10_N_RASTERS], differ;
        } a;
    };
};

// pass F-A: one workgroup per tile position.  Classes -> tokens + statistics of the class
// stream -> per raster: value statistics and Adler-32 (from per-class pixel counts and
// position weights, no raster byte is ever formed).
__global__ __launch_bounds__(kTile) void fused_stats_kernel(const FusedJob job)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    SharedFA &sh = *reinterpret_cast<SharedFA *>(smem);
    const int t = threadIdx.x;
    const uint32_t tiles = job.t.across * job.t.down;
    const uint32_t tix = blockIdx.x;
    const uint32_t ty = tix / job.t.across, tx = tix - ty * job.t.across;
    const uint8_t *class_val = job.class_of + gcn10::kClassCodes * 256;
    // (pass B adds the stream sizes up per raster and 64 positions for pass F-C's placement: from zero)
    if (job.t.chunk_tot && tix == 0u)
        for (uint32_t i = (uint32_t)t; i < job.n_sel * job.t.n_chunks; i += blockDim.x)
            job.t.chunk_tot[i] = 0u;

    for (int i = t; i < gcn10::kClassCodes * 256 / 4; i += kTile)
        reinterpret_cast<uint32_t *>(sh.class_of)[i] = reinterpret_cast<const uint32_t *>(job.class_of)[i];
    {
        const uint32_t y = ty * kTile + (uint32_t)t;
        sh.soil_row[t] = job.soil.clamp(y < job.t.rows ? (uint32_t)job.soil.cj[y] : 0u);
    }
    __syncthreads();
    load_class_tile(job, tx, ty, sh.class_of, sh.soil_row, sh.tile, t);
    __syncthreads();
    for (int i = t; i < 288; i += kTile)
        sh.a.lit_hist[i] = 0;
    if (t < 2)
        sh.a.dist_hist[t] = 0;
    sh.a.n_c[t] = 0;
    sh.a.w_c[t] = 0;
    if (t < GCN10_N_RASTERS) {
        sh.a.s1[t] = 0;
        sh.a.s2[t] = 0;
    }
    RowMasks m;
    row_masks(sh.tile, t, m);
    __syncthreads();                                // every mask is built: rows may be rewritten

    // pixels and Adler weights per class, run by run along row t (weight of byte i of the tile:
    // 65536 - i).  Runs end where the "equals its left neighbour" mask has a zero, so a row costs
    // as many steps as it has runs, not 256.
    {
        const uint8_t *row = sh.tile + t * kRowStride;
        unsigned long long brk[4] = { ~m.near_[0] | 1ull, ~m.near_[1], ~m.near_[2], ~m.near_[3] };
        const uint32_t w0 = (uint32_t)kTileBytes - (uint32_t)t * kTile;        // weight of the row's first byte
        int x0 = 0;
        while (x0 < kTile) {
            const int x1 = next_set(brk, x0 + 1);           // the next run's start, or the row's end
            const uint32_t n = (uint32_t)(x1 - x0);
            const uint32_t c = row[x0];
            atomicAdd(&sh.a.n_c[c], n);
            atomicAdd(&sh.a.w_c[c], n * w0 - ((n * (uint32_t)(x0 + x1 - 1)) >> 1));
            x0 = x1;
        }
    }
    unsigned long long start[4];
    const uint32_t my_tokens = tokenise_row(sh.tile, t, m, sh.a.lit_hist, sh.a.dist_hist, start);
    // rows back to back: where this row's tokens go
    {
        uint32_t incl = my_tokens;
        const int lane = t & 63;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off, 64);
            if (lane >= off)
                incl += up;
        }
        if (lane == 63)
            sh.a.row_base[t >> 6] = incl;
        __syncthreads();
        uint32_t at = incl - my_tokens;
        for (int w = 0; w < (t >> 6); w++)
            at += sh.a.row_base[w];
        uint16_t *out = job.tok + (size_t)tix * kTokStride;
        const uint8_t *row = sh.tile + t * kRowStride;
        int x = 0;
        while (x < kTile) {
            const int p = next_set(start, x);
            for (; x < p; x++)
                out[at++] = (uint16_t)row[x];
            if (x >= kTile)
                break;
            const uint32_t b0 = row[x], b1 = row[x + 1], b2 = row[x + 2];
            out[at++] = (uint16_t)(kTokMatch | (b0 & 31u) | (b1 & 31u) << 5 | (b0 >> 7) << 10);
            x += (int)b2 + 3;
        }
        if (t == kTile - 1) {
            out[at] = (uint16_t)kTokEnd;
            job.n_tok[tix] = at + 1u;
        }
    }
    __syncthreads();

    // Adler-32 of every raster's tile: thread t = class t, s1 = 1 + sum n_c val, s2 = N + sum w_c val;
    // and a hash of (class, value) over the classes that occur, per raster (alias detection below)
    const uint32_t lits = sh.a.lit_hist[t];
    {
        const uint32_t n = sh.a.n_c[t];
        const uint32_t w = sh.a.w_c[t] % 65521u;
        const bool present = n != 0;
        if (t < GCN10_N_RASTERS)
            sh.a.sig[t] = 0;
        if (t == 0)
            sh.a.differ = 0;
        __syncthreads();
        for (uint32_t j = 0; j < job.n_sel; j++) {
            const uint32_t v = class_val[job.sel[j] * 256 + t];
            uint32_t h = present ? (((uint32_t)t * 0x9E3779B1u + v * 0x85EBCA6Bu + 0x27D4EB2Fu) * 0x165667B1u) : 0u;
            h ^= h >> 15;
            const uint32_t p1 = wave_sum64(n * v), p2 = wave_sum64(w * v), p3 = wave_sum64(h);
            if ((t & 63) == 0) {
                atomicAdd(&sh.a.s1[j], p1);
                atomicAdd(&sh.a.s2[j], p2);
                atomicAdd(&sh.a.sig[j], p3);
            }
        }
    }
    // Rasters that cannot differ on this tile: two selected rasters whose tables map every class
    // that OCCURS here to the same value are the same bytes on it (a table's drained and undrained
    // raster wherever no dual soil class lies under the tile; all 18 on open water, ice, no-data).
    // The later raster becomes an alias of the earliest equal one.  The hash proposes the partner,
    // a comparison class by class confirms it.
    uint32_t alias_of[GCN10_N_RASTERS];
    {
        const bool present = sh.a.n_c[t] != 0;
        __syncthreads();
        if ((uint32_t)t < job.n_sel) {
            uint32_t cand = 0xffu;
            for (uint32_t q = 0; q < (uint32_t)t; q++)
                if (cand == 0xffu && sh.a.sig[q] == sh.a.sig[t])
                    cand = q;
            sh.a.cand[t] = cand;
        }
        __syncthreads();
        {
            uint32_t mine = 0;
            if (present)
                for (uint32_t j = 1; j < job.n_sel; j++) {
                    const uint32_t q = sh.a.cand[j];
                    if (q != 0xffu && class_val[job.sel[j] * 256 + t] != class_val[job.sel[q] * 256 + t])
                        mine |= 1u << j;
                }
            if (mine)
                atomicOr(&sh.a.differ, mine);
        }
        __syncthreads();
        for (uint32_t j = 0; j < job.n_sel; j++) {
            const uint32_t q = sh.a.cand[j];
            alias_of[j] = (q != 0xffu && !((sh.a.differ >> j) & 1u)) ? (kAliasFlag | q) : 0u;
        }
    }
    // per raster: literal counts by VALUE, kGroup rasters per round
    for (uint32_t j0 = 0; j0 < job.n_sel; j0 += kGroup) {
        const uint32_t nj = job.n_sel - j0 < (uint32_t)kGroup ? job.n_sel - j0 : (uint32_t)kGroup;
        for (uint32_t k = 0; k < nj; k++)
            sh.a.H[k][t] = 0;
        __syncthreads();
        if (lits)
            for (uint32_t k = 0; k < nj; k++)
                atomicAdd(&sh.a.H[k][class_val[job.sel[j0 + k] * 256 + t]], lits);
        __syncthreads();
        for (uint32_t k = 0; k < nj; k++) {
            const uint32_t j = j0 + k;
            uint32_t *out = job.t.hist + ((size_t)j * tiles + tix) * kHistWords;
            for (int i = t; i < kHistWords; i += kTile) {
                uint32_t v;
                if (i < 256)
                    v = sh.a.H[k][i];
                else if (i == 256)
                    v = 1u;                             // end of block
                else if (i < 288)
                    v = sh.a.lit_hist[i];               // match length symbols: the same for every raster
                else if (i < 290)
                    v = sh.a.dist_hist[i - 288];
                else if (i == 290)
                    v = (((65536u % 65521u + sh.a.s2[j] % 65521u) % 65521u) << 16) |
                        ((1u + sh.a.s1[j]) % 65521u);
                else if (i == 291)
                    v = alias_of[j];
                else
                    v = 0u;
                out[i] = v;
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------
// pass F-A, segment-parallel form (round 3, the default).  Same outputs as fused_stats_kernel
// -- the SAME token stream per tile position, bit for bit, and the same statistics of every raster --
// with four times the lanes: 1024 threads per tile position, ONE LANE PER 64-PIXEL SEGMENT of a
// tile row, so a lane's two match-candidate masks are one 64-bit word each and its serial walk is at
// most 64 pixels long (the row-per-lane form walks 256 pixels with four-word masks; its workgroup of
// four waves, two workgroups per CU by LDS, leaves the SIMDs two waves each -- SQ counters of round
// 2: a wave issues 42 % of the time and waits 50 %).  With 16 waves per workgroup the same 66.5 KB of
// LDS feed eight waves per SIMD.
// The greedy parse of a row is a chain (a match decides where the next token starts), and matches
// cross segment boundaries.  It is kept exact in two steps.  (1) Every lane publishes how many
// leading pixels of its segment continue a run from the segment before ("leads", for both
// distances), so a lane can tell the full length of a match that leaves its segment, and every lane
// parses its segment SPECULATIVELY from pixel 0.  (2) Segment by segment (three workgroup barriers),
// a lane reads where the last match of the segment before it really ended -- its entry offset --
// and, if that is not 0, re-parses from there only until it stands on a token start of its
// speculative parse: greedy parsing depends on the position alone, so from that pixel on the two
// parses are the same and the speculative tokens are kept (typically after one or two tokens).
// Tokens are written in raster order (row-major, segment by segment), so pass F-C, pass B and the
// host see exactly what the row form produced.
// ------------------------------------------------------------------------
constexpr int kSegs = 4;
constexpr int kSegPx = kTile / kSegs;               // 64
constexpr int kFA2Threads = kTile * kSegs;          // 1024

struct SharedFA2 {
    uint8_t tile[kTile * kRowStride];
    uint32_t soil_row[kTile];
    union {
        uint8_t class_of[gcn10::kClassCodes * 256];     // while the tile is built
        struct {
            uint32_t lit_hist[288];
            uint32_t dist_hist[2];
            uint32_t n_c[2][256], w_c[2][256];  // two copies, by lane parity: half the lanes per LDS atomic on one class
            union {
                uint32_t H[kGroup][256];                    // after the tokens are out
                struct {
                    uint32_t seg_at[kFA2Threads];           // tokens of (row, seg) in raster order, then their exclusive prefix
                    uint32_t wave_tot[kFA2Threads / 64];
                    uint8_t lead_n[kTile][kSegs];           // leading pixels of (row, seg) that continue a distance-1 run
                    uint8_t lead_f[kTile][kSegs];           // ... that equal the row above (0 .. 64)
                    uint16_t exit_at[kTile][kSegs];         // pixels by which the last match of (row, seg) overhangs it
                };
            };
            uint32_t s1[GCN10_N_RASTERS], s2[GCN10_N_RASTERS];
            uint32_t sig[GCN10_N_RASTERS], cand[GCN10_N_RASTERS], differ;
            uint32_t alias[GCN10_N_RASTERS];
        } a;
    };
};

__device__ __forceinline__ int run64(unsigned long long m, int p)
{
    // consecutive set bits of m starting at bit p (0 <= p < 64), counted to the word's end
    const unsigned long long inv = ~(m >> p);       // the bits shifted in from above are zeros: inv != 0 unless p == 0 and m is all ones
    return inv ? __builtin_ctzll(inv) : 64;
}

__global__ __launch_bounds__(kFA2Threads, 8) void fused_stats_seg_kernel(const FusedJob job)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    SharedFA2 &sh = *reinterpret_cast<SharedFA2 *>(smem);
    typedef uint32_t u32_u __attribute__((aligned(1)));
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int seg = __builtin_amdgcn_readfirstlane(t >> 8);     // a wave is 64 consecutive rows of one segment
    const int row = t & 255;
    const uint32_t tiles = job.t.across * job.t.down;
    const uint32_t tix = blockIdx.x;
    const uint32_t ty = tix / job.t.across, tx = tix - ty * job.t.across;
    const uint8_t *class_val = job.class_of + gcn10::kClassCodes * 256;
    // (pass B adds the stream sizes up per raster and 64 positions for pass F-C's placement: from zero)
    if (job.t.chunk_tot && tix == 0u)
        for (uint32_t i = (uint32_t)t; i < job.n_sel * job.t.n_chunks; i += blockDim.x)
            job.t.chunk_tot[i] = 0u;

    for (int i = t; i < gcn10::kClassCodes * 256 / 4; i += kFA2Threads)
        reinterpret_cast<uint32_t *>(sh.class_of)[i] = reinterpret_cast<const uint32_t *>(job.class_of)[i];
    if (t < kTile) {
        const uint32_t y = ty * kTile + (uint32_t)t;
        sh.soil_row[t] = job.soil.clamp(y < job.t.rows ? (uint32_t)job.soil.cj[y] : 0u);
    }
    __syncthreads();
    // class tile: thread = 4 columns x 16 rows (rows (t >> 6) + 16 i)
    {
        const uint32_t x = tx * kTile + (uint32_t)lane * 4u;
        uint32_t *dst = reinterpret_cast<uint32_t *>(sh.tile) + lane;
        const int r0 = t >> 6;
        if ((tx + 1) * kTile <= job.t.W && (ty + 1) * kTile <= job.t.rows) {
            const uint8_t *pe = job.esa + ((size_t)ty * kTile + (uint32_t)r0) * job.t.W + x;
            uint32_t e4[16], c4[16];
#pragma unroll
            for (int i = 0; i < 16; i++) {
                e4[i] = *reinterpret_cast<const u32_u *>(pe + (size_t)i * 16 * job.t.W);
                c4[i] = *reinterpret_cast<const u32_u *>(job.soil.at(sh.soil_row[r0 + 16 * i], x));
            }
#pragma unroll
            for (int i = 0; i < 16; i++) {
                uint32_t out = 0;
#pragma unroll
                for (uint32_t q = 0; q < 4; q++) {
                    const uint32_t lc = (e4[i] >> (8 * q)) & 0xffu;
                    const uint32_t cc = compact_code((c4[i] >> (8 * q)) & 0xffu);
                    out |= (uint32_t)sh.class_of[cc * 256u + lc] << (8 * q);
                }
                dst[(r0 + 16 * i) * (kRowStride / 4)] = out;
            }
        }
        else {
#pragma unroll 4
            for (int i = 0; i < 16; i++) {
                const int r = r0 + 16 * i;
                dst[r * (kRowStride / 4)] = class_pixels4(job, x, ty * kTile + (uint32_t)r, sh.class_of);
            }
        }
    }
    __syncthreads();
    for (int i = t; i < 288; i += kFA2Threads)
        sh.a.lit_hist[i] = 0;
    if (t < 2)
        sh.a.dist_hist[t] = 0;
    if (t < 256) {
        sh.a.n_c[0][t] = sh.a.n_c[1][t] = 0;
        sh.a.w_c[0][t] = sh.a.w_c[1][t] = 0;
    }
    if (t < GCN10_N_RASTERS) {
        sh.a.s1[t] = 0;
        sh.a.s2[t] = 0;
    }

    // the two candidate masks of this lane's 64 pixels
    unsigned long long near_ = 0, far_ = 0;
    const uint8_t *rowp = sh.tile + row * kRowStride;
    {
        const uint32_t *r32 = reinterpret_cast<const uint32_t *>(rowp) + seg * 16;
        const uint32_t *above = r32 - kRowStride / 4;
        uint32_t prev = seg > 0 ? r32[-1] : (row > 0 ? above[63] : 0u);      // (seg 0: the stream's previous byte is the row above's last)
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t r = r32[j];
            const uint32_t shifted = (r << 8) | (prev >> 24);
            near_ |= (unsigned long long)zero_bytes(r ^ shifted) << (4 * j);
            if (row > 0)
                far_ |= (unsigned long long)zero_bytes(r ^ above[j]) << (4 * j);
            prev = r;
        }
        if (row == 0 && seg == 0)
            near_ &= ~1ull;             // the tile's first byte has no predecessor
    }
    sh.a.lead_n[row][seg] = (uint8_t)(~near_ ? __builtin_ctzll(~near_) : kSegPx);
    sh.a.lead_f[row][seg] = (uint8_t)(~far_ ? __builtin_ctzll(~far_) : kSegPx);
    __syncthreads();

    // pixels and Adler weights per class, run by run (a run that crosses into the next segment is
    // counted in two pieces: both sums are additive)
    {
        unsigned long long brk = ~near_ | 1ull;
        const uint32_t i0 = (uint32_t)row * kTile + (uint32_t)seg * kSegPx;    // index of the segment's first byte in the tile
        while (brk) {
            const int x0 = __builtin_ctzll(brk);
            brk &= brk - 1ull;
            const int x1 = brk ? __builtin_ctzll(brk) : kSegPx;
            const uint32_t n = (uint32_t)(x1 - x0);
            const uint32_t c = rowp[seg * kSegPx + x0];
            // sum of (65536 - i) over i = i0 + x0 .. i0 + x1 - 1
            atomicAdd(&sh.a.n_c[lane & 1][c], n);
            atomicAdd(&sh.a.w_c[lane & 1][c], n * ((uint32_t)kTileBytes - i0) - ((n * (uint32_t)(x0 + x1 - 1)) >> 1));
        }
    }

    // length of the run of `far ? far_ : near_` that starts at pixel p of this segment, followed into the
    // segments behind it
    auto ext_run = [&](bool far, int p) -> int {
        int r = run64(far ? far_ : near_, p);
        if (p + r == kSegPx)
            for (int k = seg + 1; k < kSegs; k++) {
                const int l = far ? sh.a.lead_f[row][k] : sh.a.lead_n[row][k];
                r += l;
                if (l < kSegPx)
                    break;
            }
        return r;
    };
    // where a match can start: a run of >= 3 at either distance (the last two pixels look into the next segment)
    unsigned long long cand;
    {
        const uint32_t ln = seg + 1 < kSegs ? sh.a.lead_n[row][seg + 1] : 0u, lf = seg + 1 < kSegs ? sh.a.lead_f[row][seg + 1] : 0u;
        const unsigned long long n2 = ln >= 2u ? 3ull : ln, f2 = lf >= 2u ? 3ull : lf;
        cand = (near_ & ((near_ >> 1) | (n2 & 1ull) << 63) & ((near_ >> 2) | n2 << 62)) |
               (far_ & ((far_ >> 1) | (f2 & 1ull) << 63) & ((far_ >> 2) | f2 << 62));
    }
    auto span = [](int from, int to) -> unsigned long long {       // bits from .. min(to, 64) - 1
        const unsigned long long hi = to >= kSegPx ? ~0ull : (1ull << to) - 1ull;
        return hi & (~0ull << from);
    };
    // (1) speculative parse from pixel 0
    unsigned long long starts = 0, fars = 0, covered = 0;
    uint32_t exit_over = 0;
    {
        int pos = 0;
        while (pos < kSegPx) {
            const unsigned long long rest = cand >> pos;
            if (!rest)
                break;
            const int p = pos + __builtin_ctzll(rest);
            const int l1 = ext_run(false, p), l256 = ext_run(true, p);
            const bool far = l256 > l1;                 // tie: distance 1 (no extra bits)
            const int len = far ? l256 : l1;            // >= 3: bit p of cand is set
            starts |= 1ull << p;
            fars |= far ? 1ull << p : 0ull;
            covered |= span(p, p + len);
            pos = p + len;
        }
        exit_over = pos > kSegPx ? (uint32_t)(pos - kSegPx) : 0u;
    }
    // (2) the real entry offset, segment by segment
    if (seg == 0)
        sh.a.exit_at[row][0] = (uint16_t)exit_over;
    for (int sgm = 1; sgm < kSegs; sgm++) {
        __syncthreads();
        if (seg != sgm)
            continue;
        const uint32_t over = sh.a.exit_at[row][sgm - 1];
        if (over >= (uint32_t)kSegPx) {
            // the whole segment lies inside a match that started before it
            starts = fars = 0;
            covered = ~0ull;
            exit_over = over - (uint32_t)kSegPx;
        }
        else if (over > 0) {
            const unsigned long long s_tok = ~covered | starts;    // token starts of the speculative parse
            unsigned long long r_starts = 0, r_fars = 0, r_cov = (1ull << over) - 1ull;
            int pos = (int)over;
            for (;;) {
                if (pos >= kSegPx) {                    // no meeting point: the re-parse is the parse
                    starts = r_starts;
                    fars = r_fars;
                    covered = r_cov;
                    exit_over = (uint32_t)(pos - kSegPx);
                    break;
                }
                const unsigned long long tq = s_tok >> pos, rest = cand >> pos;
                const int q = tq ? pos + __builtin_ctzll(tq) : kSegPx, p = rest ? pos + __builtin_ctzll(rest) : kSegPx;
                if (q <= p) {
                    // pixels pos .. q-1 are literals; at q both parses stand on a token start: the same from there on
                    const unsigned long long hi = q < kSegPx ? ~0ull << q : 0ull;
                    starts = r_starts | (starts & hi);
                    fars = r_fars | (fars & hi);
                    covered = r_cov | (covered & hi);
                    if (q >= kSegPx)
                        exit_over = 0;
                    break;
                }
                const int l1 = ext_run(false, p), l256 = ext_run(true, p);
                const bool far = l256 > l1;
                const int len = far ? l256 : l1;
                r_starts |= 1ull << p;
                r_fars |= far ? 1ull << p : 0ull;
                r_cov |= span(p, p + len);
                pos = p + len;
            }
        }
        if (sgm + 1 < kSegs)
            sh.a.exit_at[row][sgm] = (uint16_t)exit_over;
    }
    // statistics of the final parse
    const unsigned long long lits = ~covered;
    const uint32_t my_tokens = (uint32_t)__popcll(lits) + (uint32_t)__popcll(starts);
    // (the statistics of the tokens -- literals by class, match length symbols, the two distances -- are counted where
    // the tokens are written out, below: one walk over a segment's literals and one over its matches instead of two
    // each; the scan in between needs the counts of tokens only)

    // raster order = (row, seg): an exclusive prefix over the 1024 counts says where each segment's tokens go
    sh.a.seg_at[row * kSegs + seg] = my_tokens;
    __syncthreads();
    {
        const uint32_t mine = sh.a.seg_at[t];
        uint32_t incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off, 64);
            if (lane >= off)
                incl += up;
        }
        if (lane == 63)
            sh.a.wave_tot[t >> 6] = incl;
        __syncthreads();
        uint32_t before = 0;
        for (int w = 0; w < (t >> 6); w++)
            before += sh.a.wave_tot[w];
        sh.a.seg_at[t] = before + incl - mine;
        __syncthreads();
    }
    {
        uint32_t at = sh.a.seg_at[row * kSegs + seg];
        uint16_t *out = job.tok + (size_t)tix * kTokStride;
        // Literals and matches in loops of their own (a token's place is its rank among the segment's token
        // starts): in one loop over all tokens a wave executed both paths in every trip, as often as its busiest
        // lane has tokens -- 18 of the kernel's 76 us on noisy tiles.  (Neither the LDS round trip per token nor
        // the scattered 2-byte stores were what that cost: reading ahead, or writing the tokens side by side,
        // changed nothing.)
        const unsigned long long all = lits | starts;
        for (unsigned long long m = lits; m; m &= m - 1ull) {
            const int p = __builtin_ctzll(m);
            const uint32_t c = rowp[seg * kSegPx + p];
            atomicAdd(&sh.a.lit_hist[c], 1u);
            out[at + (uint32_t)__popcll(all & ((1ull << p) - 1ull))] = (uint16_t)c;
        }
        for (unsigned long long m = starts; m; m &= m - 1ull) {
            const int p = __builtin_ctzll(m);
            const bool far = ((fars >> p) & 1ull) != 0;
            const int len = ext_run(far, p);
            uint32_t ev;                    // (no table: a global load per match inside this divergent loop)
            const int lc = length_code_extra(len, ev);
            atomicAdd(&sh.a.lit_hist[257 + lc], 1u);
            atomicAdd(&sh.a.dist_hist[far ? 1 : 0], 1u);
            out[at + (uint32_t)__popcll(all & ((1ull << p) - 1ull))] =
                (uint16_t)(kTokMatch | (uint32_t)lc | ev << 5 | (far ? 1u : 0u) << 10);
        }
        at += my_tokens;
        if (t == kFA2Threads - 1) {
            out[at] = (uint16_t)kTokEnd;
            job.n_tok[tix] = at + 1u;
        }
    }
    __syncthreads();

    // From here on the tile is no longer needed (its memory holds the value histograms below), and the work is
    // per (raster, class).  The row form does it with 256 threads, raster after raster (18 x 3 wave sums in a
    // row, three rounds of six value histograms); here the 16 waves split the rasters.
    // (a) Adler-32 sums and the (class, value) hash of every raster: wave wv takes rasters wv, wv + 16
    if (t == 0)
        sh.a.differ = 0;
    {
        const int wv = t >> 6;
        for (uint32_t j = (uint32_t)wv; j < job.n_sel; j += kFA2Threads / 64) {
            const uint8_t *val = class_val + job.sel[j] * 256;
            uint32_t a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t c = (uint32_t)lane + 64u * (uint32_t)q;
                const uint32_t n = sh.a.n_c[0][c] + sh.a.n_c[1][c];
                if (n) {
                    const uint32_t v = val[c];
                    uint32_t h = (c * 0x9E3779B1u + v * 0x85EBCA6Bu + 0x27D4EB2Fu) * 0x165667B1u;
                    h ^= h >> 15;
                    a1 += n * v;
                    a2 += ((sh.a.w_c[0][c] % 65521u + sh.a.w_c[1][c] % 65521u) % 65521u) * v;       // (<= 256 x 65520 x 255 < 2^32 over the tile)
                    a3 += h;
                }
            }
            a1 = wave_sum64(a1);
            a2 = wave_sum64(a2);
            a3 = wave_sum64(a3);
            if (lane == 0) {
                sh.a.s1[j] = a1;
                sh.a.s2[j] = a2;
                sh.a.sig[j] = a3;
            }
        }
    }
    const bool cls = t < 256;
    // (b) rasters that cannot differ on this tile (see the row form): the hash proposes, a comparison class by
    // class confirms
    {
        const bool present = cls && (sh.a.n_c[0][t] | sh.a.n_c[1][t]) != 0;
        __syncthreads();
        if ((uint32_t)t < job.n_sel) {
            uint32_t cand = 0xffu;
            for (uint32_t q = 0; q < (uint32_t)t; q++)
                if (cand == 0xffu && sh.a.sig[q] == sh.a.sig[t])
                    cand = q;
            sh.a.cand[t] = cand;
        }
        __syncthreads();
        {
            uint32_t mine = 0;
            if (present)
                for (uint32_t j = 1; j < job.n_sel; j++) {
                    const uint32_t q = sh.a.cand[j];
                    if (q != 0xffu && class_val[job.sel[j] * 256 + t] != class_val[job.sel[q] * 256 + t])
                        mine |= 1u << j;
                }
            if (mine)
                atomicOr(&sh.a.differ, mine);
        }
        __syncthreads();
        if ((uint32_t)t < job.n_sel) {
            const uint32_t q = sh.a.cand[t];
            sh.a.alias[t] = (q != 0xffu && !((sh.a.differ >> t) & 1u)) ? (kAliasFlag | q) : 0u;
        }
    }
    // (c) per raster: literal counts by VALUE, all rasters at once in the memory of the tile
    uint32_t *HV = reinterpret_cast<uint32_t *>(sh.tile);           // [n_sel][256]
    static_assert(GCN10_N_RASTERS * 256 * 4 <= kTile * kRowStride, "value histograms fit the tile's memory");
    for (uint32_t i = (uint32_t)t; i < job.n_sel * 256u; i += kFA2Threads)
        HV[i] = 0;
    __syncthreads();
    {
        const uint32_t c = (uint32_t)t & 255u;
        const uint32_t lits_c = sh.a.lit_hist[c];
        if (lits_c)
            for (uint32_t j = (uint32_t)t >> 8; j < job.n_sel; j += kFA2Threads / 256)
                atomicAdd(&HV[j * 256u + class_val[job.sel[j] * 256 + c]], lits_c);
    }
    __syncthreads();
    for (uint32_t idx = (uint32_t)t; idx < job.n_sel * (uint32_t)kHistWords; idx += kFA2Threads) {
        const uint32_t j = idx / (uint32_t)kHistWords;
        const int i = (int)(idx - j * (uint32_t)kHistWords);
        uint32_t v;
        if (i < 256)
            v = HV[j * 256u + (uint32_t)i];
        else if (i == 256)
            v = 1u;                             // end of block
        else if (i < 288)
            v = sh.a.lit_hist[i];               // match length symbols: the same for every raster
        else if (i < 290)
            v = sh.a.dist_hist[i - 288];
        else if (i == 290)
            v = (((65536u % 65521u + sh.a.s2[j] % 65521u) % 65521u) << 16) | ((1u + sh.a.s1[j]) % 65521u);
        else if (i == 291)
            v = sh.a.alias[j];
        else
            v = 0u;
        job.t.hist[((size_t)j * tiles + tix) * kHistWords + i] = v;
    }
}

// Pass F-A for every tile position of the job, in the form opt.fused_parse names.  (A launch error shows at the
// check behind pass B, the next launch.)
int launch_fused_stats(gcn10_gpu_ctx *ctx, const FusedJob &job, hipStream_t s)
{
    static_assert(sizeof(SharedFA) <= 80 * 1024, "two fused statistics workgroups per CU");
    static_assert(sizeof(SharedFA2) <= 80 * 1024, "two segment-parallel statistics workgroups (32 waves) per CU");
    if (!ctx->fused_stats_ready) {
        HIP_TRY(gcn10::allow_dynamic_lds(fused_stats_kernel, sizeof(SharedFA)));
        HIP_TRY(gcn10::allow_dynamic_lds(fused_stats_seg_kernel, sizeof(SharedFA2)));
        ctx->fused_stats_ready = true;
    }
    const uint32_t positions = job.t.across * job.t.down;
    if (ctx->opt.fused_parse == 0)
        hipLaunchKernelGGL(fused_stats_kernel, dim3(positions), dim3(kTile), sizeof(SharedFA), s, job);
    else
        hipLaunchKernelGGL(fused_stats_seg_kernel, dim3(positions), dim3(kFA2Threads), sizeof(SharedFA2), s, job);
    return GCN10_OK;
}

}  // namespace

#endif
