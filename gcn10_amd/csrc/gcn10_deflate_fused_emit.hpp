// gcn10_deflate_fused_emit.hpp -- pass F-C of the fused tile encoder (included by gcn10_deflate_fused.hip alone):
// one workgroup per (tile position, group of kGroup rasters) turns the position's tokens into the group's streams.
// Two forms with the same streams, bit for bit: every wave packs its own quarter of the tokens and the workgroup
// places its streams itself (fused_emit_wave_kernel, the default), and four waves in lock step behind pass B'
// (fused_emit_kernel, option fused_emit = 0, the cross-check).  launch_fused_emit picks the form.
#ifndef GCN10_DEFLATE_FUSED_EMIT_HPP
#define GCN10_DEFLATE_FUSED_EMIT_HPP

#include "gcn10_deflate_fused_internal.hpp"

using gcn10::u32x4;
using gcn10::wave_scan;

namespace {

constexpr int kStageWords = 88;         // 64 tokens x 41 bits, starting anywhere in the first word

struct SharedFC {
    union {
        struct {
            uint32_t cl[288][8];            // code | length << 16 of the group's rasters, by class / length symbol
            uint32_t stage[4][kGroup][kStageWords];     // per wave: the bits of its 64 tokens, per raster
        } c;
        uint8_t class_of[gcn10::kClassCodes * 256];     // stored fallback only, after the streams
    };
    uint32_t wave_tot[kGroup / 2][4];       // bits of each wave's tokens, two streams per word
    uint32_t masks[2];
};

// pass F-C: one workgroup per (tile position, group of kGroup rasters), token-parallel.
// Every thread takes one token of the position's stream per trip, looks up the group's codes
// for it (one LDS read), a prefix sum over the workgroup gives its bit position in each of
// the kGroup streams, the bits are OR-ed into a per-wave staging area in LDS and go to the
// arena as whole words (the first and last word of a wave's span are OR-ed into the zeroed
// slot, the words in between are plain coalesced stores).  No row walk, no divergence: the
// work is the number of tokens, whatever their distribution over the rows.
__global__ __launch_bounds__(kTile) void fused_emit_kernel(const FusedJob job)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    SharedFC &sh = *reinterpret_cast<SharedFC *>(smem);
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);        // wave-uniform: selects on it stay scalar
    const uint32_t tiles = job.t.across * job.t.down;
    const uint32_t tix = blockIdx.x;
    const uint32_t ty = tix / job.t.across, tx = tix - ty * job.t.across;
    const uint32_t j0 = blockIdx.y * kGroup;
    const uint32_t nj = job.n_sel - j0 < (uint32_t)kGroup ? job.n_sel - j0 : (uint32_t)kGroup;
    const uint8_t *class_val = job.class_of + gcn10::kClassCodes * 256;

    // which rasters of the group have a slot, and which of those are stored
    uint32_t live, stored_mask;
    {
        int mine = 0, st = 0;
        if ((uint32_t)t < nj) {
            const Book *b = reinterpret_cast<const Book *>(job.t.books + ((size_t)(j0 + t) * tiles + tix) * kBookBytes);
            mine = job.t.table[((size_t)(j0 + t) * tiles + tix) * 2] < kAliasSlot;      // neither "arena too small" nor an alias
            st = mine && b->stream_bytes == (uint32_t)kMaxStream;
            // an alias's table entry is its original's (written by pass B, a launch ago)
            const uint32_t al = job.t.hist[((size_t)(j0 + t) * tiles + tix) * kHistWords + 291];
            if (al & kAliasFlag) {
                const size_t from = ((size_t)(al & 0xffu) * tiles + tix) * 2, to = ((size_t)(j0 + t) * tiles + tix) * 2;
                job.t.table[to] = job.t.table[from];
                job.t.table[to + 1] = job.t.table[from + 1];
            }
        }
        live = (uint32_t)__ballot(mine);            // threads t < nj are all in wave 0: its ballots are the
        stored_mask = (uint32_t)__ballot(st);       // masks, the other waves get them through LDS
        if (t == 0) {
            sh.masks[0] = live;
            sh.masks[1] = stored_mask;
        }
        __syncthreads();
        live = sh.masks[0];
        stored_mask = sh.masks[1];
        if (live == 0)
            return;
    }
    const uint32_t coded = live & ~stored_mask;     // rasters that get a Huffman stream

    // codes of the group's rasters by class (a literal of class c is the symbol val(c)), the
    // zeroed slots with their block headers, and per raster what is the same for every token
    uint32_t *words[kGroup];
    uint32_t base[kGroup], dcode0[kGroup], dlen0[kGroup], dcode1[kGroup], dlen1[kGroup];
#pragma unroll
    for (int k = 0; k < kGroup; k++) {
        words[k] = nullptr;
        base[k] = dcode0[k] = dlen0[k] = dcode1[k] = dlen1[k] = 0;
        if (!((coded >> k) & 1u))
            continue;
        const uint32_t j = j0 + k;
        const Book *b = reinterpret_cast<const Book *>(job.t.books + ((size_t)j * tiles + tix) * kBookBytes);
        words[k] = reinterpret_cast<uint32_t *>(job.t.arena + job.t.table[((size_t)j * tiles + tix) * 2]);
        base[k] = b->header_bits;
        dcode0[k] = b->dist_code[0];
        dlen0[k] = b->dist_len[0];
        dcode1[k] = (uint32_t)b->dist_code[1] | 63u << b->dist_len[1];      // + 6 extra bits: 256 - 193
        dlen1[k] = (uint32_t)b->dist_len[1] + 6u;
        // (up to the slot's 16-byte end: the host writes a raster's streams of a strip as one extent,
        // the few bytes between two streams included -- they are zeros, not whatever the arena held)
        const uint32_t n_words = (b->stream_bytes + 15u) / 16u * 4u;
        for (uint32_t i = t; i < n_words; i += kTile)
            words[k][i] = i < 64u ? b->header[i] : 0u;
        for (int i = t; i < 288; i += kTile) {
            const uint32_t sym = i < 256 ? class_val[job.sel[j] * 256 + i] : (uint32_t)i;
            sh.c.cl[i][k] = (uint32_t)b->lit_code[sym] | (uint32_t)b->lit_len[sym] << 16;
        }
    }
    for (int i = t; i < 4 * kGroup * kStageWords; i += kTile)
        (&sh.c.stage[0][0][0])[i] = 0u;
    __threadfence_block();                          // the zeroed slots are in place before this workgroup ORs into them
    __syncthreads();

    if (coded) {
        const uint16_t *tok = job.tok + (size_t)tix * kTokStride;
        const uint32_t n_tok = job.n_tok[tix];
        for (uint32_t i0 = 0; i0 < n_tok; i0 += kTile) {
            const uint32_t i = i0 + (uint32_t)t;
            const bool have = i < n_tok;
            const uint32_t tk = have ? tok[i] : 0u;
            const bool is_match = (tk & kTokMatch) != 0;
            const uint32_t sym = is_match ? 257u + (tk & 31u) : (tk & kTokEnd) ? 256u : (tk & 255u);
            const uint32_t lc = tk & 31u;
            const uint32_t ne = !is_match || lc < 8u || lc == 28u ? 0u : (lc - 4u) >> 2;
            const uint32_t ev = is_match ? (tk >> 5) & 31u : 0u;
            const bool far = ((tk >> 10) & 1u) != 0;
            const u32x4 c03 = *reinterpret_cast<const u32x4 *>(&sh.c.cl[sym][0]);
            const u32x4 c47 = *reinterpret_cast<const u32x4 *>(&sh.c.cl[sym][4]);
            // the token's bits in every stream of the group: at most 15 + 5 + 15 + 6 = 41
            uint32_t lo[kGroup], hi[kGroup], n[kGroup];
#pragma unroll
            for (int k = 0; k < kGroup; k++) {
                const uint32_t c = k < 4 ? c03[k] : c47[k - 4];
                const uint32_t l = c >> 16;
                const uint32_t nb = l + ne;                         // <= 20
                const uint32_t d = is_match ? (far ? dcode1[k] : dcode0[k]) : 0u;
                const uint32_t dl = is_match ? (far ? dlen1[k] : dlen0[k]) : 0u;
                lo[k] = (c & 0xffffu) | ev << l | d << nb;
                hi[k] = (d >> 1) >> (31u - nb);
                n[k] = have && ((coded >> k) & 1u) ? nb + dl : 0u;
            }
            // prefix sums over the wave, two streams per register (a wave's total is < 2^16)
            uint32_t excl[kGroup];
#pragma unroll
            for (int k = 0; k < kGroup; k += 2) {
                const uint32_t mine = n[k] | n[k + 1] << 16;
                const uint32_t incl = wave_scan(mine);
                const uint32_t ex = incl - mine;
                excl[k] = ex & 0xffffu;
                excl[k + 1] = ex >> 16;
                if (lane == 63)
                    sh.wave_tot[k / 2][wave] = incl;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kGroup; k++) {
                if (!((coded >> k) & 1u))
                    continue;
                const int h = 16 * (k & 1);
                const uint32_t t0 = (sh.wave_tot[k / 2][0] >> h) & 0xffffu, t1 = (sh.wave_tot[k / 2][1] >> h) & 0xffffu,
                               t2 = (sh.wave_tot[k / 2][2] >> h) & 0xffffu, t3 = (sh.wave_tot[k / 2][3] >> h) & 0xffffu;
                const uint32_t before = wave == 0 ? 0u : wave == 1 ? t0 : wave == 2 ? t0 + t1 : t0 + t1 + t2;
                const uint32_t mine = wave == 0 ? t0 : wave == 1 ? t1 : wave == 2 ? t2 : t3;
                const uint32_t first = base[k] + before;            // this wave's first bit in the stream
                const uint32_t word0 = first >> 5;
                uint32_t *stage = sh.c.stage[wave][k];
                {
                    // 41 bits shifted by up to 31: three words, OR-ed unconditionally (absent tokens are zeros)
                    const uint32_t rel = (first & 31u) + excl[k];
                    const uint32_t w = rel >> 5, sft = rel & 31u;
                    const uint32_t l32 = n[k] ? lo[k] : 0u, h32 = n[k] ? hi[k] : 0u;
                    atomicOr(&stage[w], l32 << sft);
                    atomicOr(&stage[w + 1], (l32 >> 1) >> (31u - sft) | h32 << sft);
                    atomicOr(&stage[w + 2], (h32 >> 1) >> (31u - sft));
                }
                // (one wave: the LDS atomics above are complete before the reads below issue)
                const uint32_t n_words = ((first & 31u) + mine + 31u) >> 5;
                for (uint32_t w = (uint32_t)lane; w < n_words; w += 64u) {
                    const uint32_t val = stage[w];
                    stage[w] = 0u;
                    if (w == 0u || w == n_words - 1u)
                        atomicOr(&words[k][word0 + w], val);
                    else
                        words[k][word0 + w] = val;
                }
                base[k] += t0 + t1 + t2 + t3;
            }
            __syncthreads();                        // wave_tot is rewritten in the next trip
        }
    }
    // trailers: the Adler-32 of the raster's tile, big endian, after the last (padded) byte
    if ((uint32_t)t < nj && ((coded >> t) & 1u)) {
        const uint32_t j = j0 + (uint32_t)t;
        const Book *b = reinterpret_cast<const Book *>(job.t.books + ((size_t)j * tiles + tix) * kBookBytes);
        const uint32_t adler = job.t.hist[((size_t)j * tiles + tix) * kHistWords + 290];
        uint32_t *w = reinterpret_cast<uint32_t *>(job.t.arena + job.t.table[((size_t)j * tiles + tix) * 2]);
        const uint32_t at = b->stream_bytes - 4u;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            const uint32_t byte = (adler >> (24 - 8 * i)) & 0xffu;
            atomicOr(&w[(at + i) >> 2], byte << (8 * ((at + i) & 3u)));
        }
    }
    if (stored_mask == 0)
        return;

    // stored fallback (incompressible tiles): the raster's bytes are val(class), two blocks of
    // 32768 bytes; the classes are formed again from landcover + soil
    __syncthreads();
    for (int i = t; i < gcn10::kClassCodes * 256 / 4; i += kTile)
        reinterpret_cast<uint32_t *>(sh.class_of)[i] = reinterpret_cast<const uint32_t *>(job.class_of)[i];
    __syncthreads();
    for (uint32_t k = 0; k < nj; k++) {
        if (!((stored_mask >> k) & 1u))
            continue;
        const uint32_t j = j0 + k;
        uint8_t *o = job.t.arena + job.t.table[((size_t)j * tiles + tix) * 2];
        const uint32_t adler = job.t.hist[((size_t)j * tiles + tix) * kHistWords + 290];
        if (t == 0) {
            o[0] = 0x78;
            o[1] = 0x01;
            for (int blk = 0; blk < 2; blk++) {
                uint8_t *h = o + 2 + blk * (5 + 32768);
                h[0] = (uint8_t)(blk == 1);
                h[1] = 0x00;
                h[2] = 0x80;
                h[3] = 0xff;
                h[4] = 0x7f;
            }
            const uint32_t at = (uint32_t)kMaxStream - 4u;
            o[at] = (uint8_t)(adler >> 24);
            o[at + 1] = (uint8_t)(adler >> 16);
            o[at + 2] = (uint8_t)(adler >> 8);
            o[at + 3] = (uint8_t)adler;
        }
        const uint8_t *val = class_val + job.sel[j] * 256;
        const uint32_t xc = (uint32_t)(t & 63) * 4u;
        for (int i = 0; i < kTile / 4; i++) {
            const int r = i * 4 + (t >> 6);
            const uint32_t c4 = class_pixels4(job, tx * kTile + xc, ty * kTile + (uint32_t)r, sh.class_of);
            uint8_t *dst = o + 2 + (r >> 7) * (5 + 32768) + 5 + (r & 127) * kTile + xc;
            dst[0] = val[c4 & 0xffu];
            dst[1] = val[(c4 >> 8) & 0xffu];
            dst[2] = val[(c4 >> 16) & 0xffu];
            dst[3] = val[c4 >> 24];
        }
    }
}

// ------------------------------------------------------------------------
// pass F-C, wave-independent form (round 3, the default).  Same streams as fused_emit_kernel, bit for
// bit.  That kernel walks the token stream 256 tokens per trip with all four waves in lock step, one
// token per lane, and ORs every token's bits into LDS staging words with three 32-bit atomics per
// stream.  Timing switches (profiles/r03) put its time in two places: LDS atomics whose lanes hit the
// same word (a token is ~8 bits: eight neighbouring lanes per 64-bit word, executed one after the
// other) and the write-out of ~20 staged words per stream and trip behind them -- with the next trip's
// token load queued behind those stores (vmcnt is one in-order queue).  Here
//   * every wave owns one contiguous QUARTER of the position's tokens: phase 1 adds up the bits its
//     quarter takes in each of the group's streams (no packing), ONE workgroup barrier, and the sums
//     before it say where the wave's bits begin in every stream; nothing is shared after that;
//   * a lane takes FOUR consecutive tokens and packs their codes into a register chunk (<= 164 bits)
//     before anything touches LDS: a wave's trip is 256 tokens, a lane's chunk is ~40 bits, so at most
//     two lanes meet in a 64-bit staging word and there are a quarter of the atomics;
//   * the group's six codes of a class are ONE 16-byte LDS row (20 bits per stream: code | length << 15);
//   * the next trip's tokens are loaded before this trip's words are stored.
// ------------------------------------------------------------------------
constexpr int kLaneToks = 4;                        // consecutive tokens per lane and trip
constexpr int kTripToks = 64 * kLaneToks;           // 256 tokens per wave and trip
constexpr int kStage64 = (63 + kTripToks * 41 + 63) / 64 + 2;      // a trip's bits starting anywhere in the first word: 166 words

struct SharedFC2 {
    union {
        struct {
            unsigned long long cl[288][2];                          // 20 bits per stream: code | length << 15; streams 0-2, 3-5
            unsigned long long stage[4][kStage64];                  // per wave: the bits of one trip of one stream
        } c;
        uint8_t class_of[gcn10::kClassCodes * 256];                 // stored fallback only, after the streams
    };
    uint32_t chunk_bits[kGroup][4];         // bits of each wave's quarter, per stream
    uint32_t masks[2];
    uint32_t r_tot[GCN10_N_RASTERS];        // arena bytes of every raster's streams of this strip (16-byte slots)
    uint32_t r_pre[GCN10_N_RASTERS];        // ... of its positions before this one
    uint32_t slot[kGroup];                  // where this position's streams of the group lie
};

// what a 16-bit token says: symbol, extra bits of a length, which distance
struct TokFields {
    uint32_t sym, ne, ev;
    bool is_match, far;
};

__device__ __forceinline__ TokFields tok_fields(uint32_t tk)
{
    TokFields f;
    f.is_match = (tk & kTokMatch) != 0;
    const uint32_t lc = tk & 31u;
    f.sym = f.is_match ? 257u + lc : (tk & kTokEnd) ? 256u : (tk & 255u);
    f.ne = !f.is_match || lc < 8u || lc == 28u ? 0u : (lc - 4u) >> 2;
    f.ev = f.is_match ? (tk >> 5) & 31u : 0u;
    f.far = ((tk >> 10) & 1u) != 0;
    return f;
}

// code | length << 15 of stream k (0..5) from the two halves of a cl row
__device__ __forceinline__ uint32_t cl_field(unsigned long long h0, unsigned long long h1, int k)
{
    return (uint32_t)((k < 3 ? h0 : h1) >> (20 * (k % 3))) & 0xfffffu;
}

__global__ __launch_bounds__(kTile, 6) void fused_emit_wave_kernel(const FusedJob job)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    SharedFC2 &sh = *reinterpret_cast<SharedFC2 *>(smem);
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const uint32_t tiles = job.t.across * job.t.down;
    const uint32_t tix = blockIdx.x;
    const uint32_t ty = tix / job.t.across, tx = tix - ty * job.t.across;
    const uint32_t j0 = blockIdx.y * kGroup;
    const uint32_t nj = job.n_sel - j0 < (uint32_t)kGroup ? job.n_sel - j0 : (uint32_t)kGroup;
    const uint8_t *class_val = job.class_of + gcn10::kClassCodes * 256;

    // Where this position's streams go (round 3: pass B' folded in -- a launch of one workgroup and its kernel
    // boundary were 16-18 us per strip).  Pass B left sizes[i] = { alias mark or 0, stream bytes } and added every
    // stream's 16-byte-aligned size to chunk_tot[raster][position / 64].  The layout is raster-major, tiles of a
    // raster in order, 16-byte slots, every raster's extent starting at a multiple of seg_align (a power of two):
    // the offset of (raster j, this position) is the sum of the aligned totals of the rasters before j plus the sizes
    // of raster j's earlier positions.  Every workgroup adds those up for itself: the chunk totals of the rasters up
    // to its own (one load per lane for a 1024-row strip of a 3-degree block: 18 x 9 values) and the sizes of its own
    // chunk of positions (at most 4.5 loads per lane) -- one memory latency, against the 61 KB table a workgroup
    // would otherwise have to read.  It writes the offsets of ITS six streams into the table for the host and keeps
    // them in LDS for itself.  The workgroups of position 0 zero the pads in front of their rasters' extents; the one
    // of the last group also writes the bytes used.
    {
        const uint32_t jn = j0 + nj;                    // (an alias's original is an earlier raster, maybe of another group)
        const uint32_t chunks = job.t.n_chunks, c = tix >> 6;
        if (t < GCN10_N_RASTERS) {
            sh.r_tot[t] = 0;
            sh.r_pre[t] = 0;
        }
        __syncthreads();
        for (uint32_t i = (uint32_t)t; i < jn * chunks; i += (uint32_t)kTile) {
            const uint32_t v = job.t.chunk_tot[i];
            const uint32_t r = i / chunks, cc = i - r * chunks;
            if (v) {
                atomicAdd(&sh.r_tot[r], v);
                if (cc < c)
                    atomicAdd(&sh.r_pre[r], v);
            }
        }
        const uint2 *tab = reinterpret_cast<const uint2 *>(job.t.sizes);
        for (uint32_t r = (uint32_t)wave; r < jn; r += 4u) {
            const uint32_t pp = c * 64u + (uint32_t)lane;
            uint32_t nd = 0;
            if (pp < tix) {
                const uint2 e = tab[(size_t)r * tiles + pp];
                nd = e.x == kAliasSlot ? 0u : (e.y + (uint32_t)(kSlotAlign - 1)) & ~(uint32_t)(kSlotAlign - 1);
            }
            nd = wave_scan(nd);
            if (lane == 63 && nd)
                atomicAdd(&sh.r_pre[r], nd);
        }
    }
    __syncthreads();
    // which rasters of the group have a slot, and which of those are stored
    uint32_t live, stored_mask;
    {
        int mine = 0, st = 0;
        if (wave == 0) {
            // extents: seg[j] = sum over r < j of the aligned totals (a scan over lanes 0..17)
            const unsigned long long am = (unsigned long long)job.seg_align - 1ull;
            const unsigned long long tot = (uint32_t)lane < job.n_sel ? sh.r_tot[lane] : 0u;
            unsigned long long incl = (tot + am) & ~am;
#pragma unroll
            for (int off = 1; off < 32; off <<= 1) {
                const unsigned long long up = __shfl_up(incl, off, 64);
                if (lane >= off)
                    incl += up;
            }
            const unsigned long long seg = incl - ((tot + am) & ~am);      // where raster `lane`'s extent starts
            const bool own = (uint32_t)t < nj;
            const uint32_t j = own ? j0 + (uint32_t)t : 0u;
            const uint32_t al = own ? job.t.hist[((size_t)j * tiles + tix) * kHistWords + 291] : 0u;
            // an alias's table entry is its original's; the original may belong to another group's workgroup, so its
            // offset is worked out here as well
            const uint32_t src_j = al & kAliasFlag ? (al & 0xffu) : j;
            const unsigned long long src_seg = __shfl(seg, (int)src_j, 64);
            if (own) {
                const size_t to = ((size_t)j * tiles + tix) * 2;
                const Book *b = reinterpret_cast<const Book *>(job.t.books + ((size_t)j * tiles + tix) * kBookBytes);
                const uint32_t bytes = al & kAliasFlag ? job.t.sizes[((size_t)src_j * tiles + tix) * 2 + 1] : b->stream_bytes;
                const unsigned long long off = src_seg + sh.r_pre[src_j];
                const uint32_t need = (bytes + (uint32_t)(kSlotAlign - 1)) & ~(uint32_t)(kSlotAlign - 1);
                const bool fits = off + need <= job.t.arena_cap;
                job.t.table[to] = fits ? (uint32_t)off : 0xffffffffu;
                job.t.table[to + 1] = fits ? bytes : 0u;
                sh.slot[t] = fits ? (uint32_t)off : 0xffffffffu;
                mine = !(al & kAliasFlag) && fits;       // neither "arena too small" nor an alias
                st = mine && bytes == (uint32_t)kMaxStream;
            }
            if (tix == 0u) {
                // pads: behind each of my rasters' last stream up to the next extent's start (behind the last raster:
                // up to the next multiple of the alignment: an O_DIRECT write reads that far); *cursor = bytes used
                for (uint32_t k = 0; k < nj; k++) {
                    const uint32_t r = j0 + k;
                    const unsigned long long from = __shfl(seg, (int)r, 64) + __shfl(tot, (int)r, 64);
                    unsigned long long to = (from + am) & ~am;
                    if (to > job.t.arena_cap)
                        to = job.t.arena_cap;
                    for (unsigned long long o = from + (unsigned long long)lane * 16u; o + 16u <= to; o += 64u * 16u)
                        *reinterpret_cast<u32x4 *>(job.t.arena + o) = u32x4{ 0u, 0u, 0u, 0u };
                    if (r + 1u == job.n_sel && lane == 0)
                        *job.t.cursor = from;
                }
            }
        }
        live = (uint32_t)__ballot(mine);
        stored_mask = (uint32_t)__ballot(st);
        if (t == 0) {
            sh.masks[0] = live;
            sh.masks[1] = stored_mask;
        }
        __syncthreads();
        live = sh.masks[0];
        stored_mask = sh.masks[1];
        if (live == 0)
            return;
    }
    const uint32_t coded = __builtin_amdgcn_readfirstlane(live & ~stored_mask);     // rasters that get a Huffman stream

    // per stream: where it lies, where its tokens begin, its two distance codes (wave-uniform: scalar registers)
    unsigned long long *words[kGroup];
    uint32_t base[kGroup], dcode0[kGroup], dlen0[kGroup], dcode1[kGroup], dlen1[kGroup];
    for (int i = t; i < 288 * 2; i += kTile)
        (&sh.c.cl[0][0])[i] = 0ull;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kGroup; k++) {
        words[k] = nullptr;
        base[k] = dcode0[k] = dlen0[k] = dcode1[k] = dlen1[k] = 0;
        if (!((coded >> k) & 1u))
            continue;
        const uint32_t j = j0 + k;
        const Book *b = reinterpret_cast<const Book *>(job.t.books + ((size_t)j * tiles + tix) * kBookBytes);
        uint32_t *w32 = reinterpret_cast<uint32_t *>(job.t.arena + sh.slot[k]);
        words[k] = reinterpret_cast<unsigned long long *>(w32);
        base[k] = __builtin_amdgcn_readfirstlane(b->header_bits);
        dcode0[k] = __builtin_amdgcn_readfirstlane((uint32_t)b->dist_code[0]);
        dlen0[k] = __builtin_amdgcn_readfirstlane((uint32_t)b->dist_len[0]);
        dcode1[k] = __builtin_amdgcn_readfirstlane((uint32_t)b->dist_code[1] | 63u << b->dist_len[1]);     // + 6 extra bits: 256 - 193
        dlen1[k] = __builtin_amdgcn_readfirstlane((uint32_t)b->dist_len[1] + 6u);
        // the zeroed slot with its block header, up to the slot's 16-byte end (the host writes a raster's
        // streams of a strip as one extent: the bytes between two streams are zeros)
        const uint32_t n_words = (b->stream_bytes + 15u) / 16u * 4u;
        for (uint32_t i = t; i < n_words; i += kTile)
            w32[i] = i < 64u ? b->header[i] : 0u;
        // (k-th 20-bit field of its half: every (i, k) is touched by one thread, the halves were zeroed above)
        for (int i = t; i < 288; i += kTile) {
            const uint32_t sym = i < 256 ? class_val[job.sel[j] * 256 + i] : (uint32_t)i;
            const unsigned long long f = (unsigned long long)((uint32_t)b->lit_code[sym] | (uint32_t)b->lit_len[sym] << 15);
            sh.c.cl[i][k / 3] |= f << (20 * (k % 3));
        }
    }
    for (int i = t; i < 4 * kStage64; i += kTile)
        (&sh.c.stage[0][0])[i] = 0ull;

    const uint16_t *tok = job.tok + (size_t)tix * kTokStride;
    const uint32_t n_tok = coded ? job.n_tok[tix] : 0u;
    // this wave's quarter: whole trips of 256 tokens
    const uint32_t per_wave = ((n_tok + 4u * kTripToks - 1u) / (4u * kTripToks)) * kTripToks;
    const uint32_t c0 = (uint32_t)wave * per_wave;
    const uint32_t c1 = c0 + per_wave < n_tok ? c0 + per_wave : n_tok;
    __threadfence_block();                          // the zeroed slots are in place before this workgroup ORs into them
    __syncthreads();

    // four consecutive tokens of this lane (8-byte aligned: kTokStride and the trips are multiples of 4)
    auto load4 = [&](uint32_t i0) -> uint2 {
        const uint32_t i = i0 + (uint32_t)lane * kLaneToks;
        return i < c1 ? *reinterpret_cast<const uint2 *>(tok + i) : make_uint2(0u, 0u);
    };
    auto tok_of = [](uint2 v, int q) -> uint32_t { return ((q < 2 ? v.x : v.y) >> (16 * (q & 1))) & 0xffffu; };

    // phase 1: the bits of this quarter in every stream
    {
        uint32_t acc[kGroup];
#pragma unroll
        for (int k = 0; k < kGroup; k++)
            acc[k] = 0;
        for (uint32_t i0 = c0; i0 < c1; i0 += kTripToks) {
            const uint2 v = load4(i0);
#pragma unroll
            for (int q = 0; q < kLaneToks; q++) {
                if (i0 + (uint32_t)lane * kLaneToks + (uint32_t)q >= c1)
                    continue;
                const TokFields f = tok_fields(tok_of(v, q));
                const unsigned long long h0 = sh.c.cl[f.sym][0], h1 = sh.c.cl[f.sym][1];
#pragma unroll
                for (int k = 0; k < kGroup; k++)
                    acc[k] += (cl_field(h0, h1, k) >> 15) + f.ne + (f.is_match ? (f.far ? dlen1[k] : dlen0[k]) : 0u);
            }
        }
#pragma unroll
        for (int k = 0; k < kGroup; k++) {
            const uint32_t tot = wave_scan(acc[k]);
            if (lane == 63)
                sh.chunk_bits[k][wave] = (coded >> k) & 1u ? tot : 0u;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kGroup; k++) {
        const uint32_t b0 = sh.chunk_bits[k][0], b1 = sh.chunk_bits[k][1], b2 = sh.chunk_bits[k][2];
        base[k] += wave == 0 ? 0u : wave == 1 ? b0 : wave == 2 ? b0 + b1 : b0 + b1 + b2;
        base[k] = __builtin_amdgcn_readfirstlane(base[k]);
    }

    // phase 2: 256 tokens per trip, this wave alone
    unsigned long long *stage = sh.c.stage[wave];
    unsigned long long carry[kGroup];               // per stream: the unfinished last word of the previous trip (wave-uniform)
#pragma unroll
    for (int k = 0; k < kGroup; k++)
        carry[k] = 0ull;
    uint2 next = load4(c0);
    for (uint32_t i0 = c0; i0 < c1; i0 += kTripToks) {
        const uint2 v = next;
        next = load4(i0 + kTripToks);               // (in front of this trip's stores: vmcnt is one in-order queue)
        TokFields f[kLaneToks];
        unsigned long long h0[kLaneToks], h1[kLaneToks];
        bool have[kLaneToks];
#pragma unroll
        for (int q = 0; q < kLaneToks; q++) {
            have[q] = i0 + (uint32_t)lane * kLaneToks + (uint32_t)q < c1;
            f[q] = tok_fields(have[q] ? tok_of(v, q) : 0u);         // (past the end: a harmless symbol, no bits)
            h0[q] = sh.c.cl[f[q].sym][0];
            h1[q] = sh.c.cl[f[q].sym][1];
        }
#pragma unroll
        for (int k = 0; k < kGroup; k++) {
            if (!((coded >> k) & 1u))
                continue;
            // the lane's four tokens packed into a chunk of <= 4 x 41 = 164 bits
            unsigned long long a0 = 0, a1 = 0, a2 = 0;
            uint32_t off = 0;
#pragma unroll
            for (int q = 0; q < kLaneToks; q++) {
                const uint32_t c = cl_field(h0[q], h1[q], k);
                const uint32_t l = c >> 15;
                const uint32_t nb = l + f[q].ne;                        // <= 20
                const uint32_t d = f[q].is_match ? (f[q].far ? dcode1[k] : dcode0[k]) : 0u;
                const uint32_t dl = f[q].is_match ? (f[q].far ? dlen1[k] : dlen0[k]) : 0u;
                const uint32_t n = have[q] ? nb + dl : 0u;
                const unsigned long long bits = n ? (unsigned long long)((c & 0x7fffu) | f[q].ev << l) | (unsigned long long)d << nb : 0ull;
                // off <= 41 q: the token starts in word 0 or 1 of the chunk
                const uint32_t s = off & 63u;
                const unsigned long long lo = bits << s, hi = (bits >> 1) >> (63u - s);
                if (q == 0) {
                    a0 = bits;
                }
                else if (q == 1) {                  // off <= 41
                    a0 |= lo;
                    a1 |= hi;
                }
                else {                              // off <= 123
                    const bool w1 = off >= 64u;
                    a0 |= w1 ? 0ull : lo;
                    a1 |= w1 ? lo : hi;
                    a2 |= w1 ? hi : 0ull;
                }
                off += n;
            }
            // where the chunk goes: prefix sum of the lanes' bit counts (a trip's total is < 2^16)
            const uint32_t incl = wave_scan(off);
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            const uint32_t first = base[k];                             // this trip's first bit in the stream (wave-uniform)
            // the unfinished last word of this stream's previous trip is the first word of this one
            if (lane == 0)
                stage[0] = carry[k];
            {
                const uint32_t rel = (first & 63u) + incl - off;
                const uint32_t w = rel >> 6, s = rel & 63u;
                const unsigned long long v0 = a0 << s, v1 = a1 << s | (a0 >> 1) >> (63u - s),
                                         v2 = a2 << s | (a1 >> 1) >> (63u - s), v3 = (a2 >> 1) >> (63u - s);
                if (v0) atomicOr(&stage[w], v0);
                if (v1) atomicOr(&stage[w + 1], v1);
                if (v2) atomicOr(&stage[w + 2], v2);
                if (v3) atomicOr(&stage[w + 3], v3);
            }
            // (one wave: LDS executes its instructions in order, the reads below see the atomics above)
            // Words of this trip: the last one, if the trip does not end on a word boundary, stays with the wave
            // (carry) -- except in the wave's last trip -- so that only the first word of a wave's first trip and
            // the last word of its last trip are shared with anyone (the header, a neighbouring wave, the trailer)
            // and need a global atomic; everything else is a plain 8-byte store.  (Two atomics per word-sharing
            // trip were 0.10 of this kernel's 0.15 ms per noisy strip: profiles/r03.)
            const uint32_t end = (first & 63u) + total;
            const uint32_t n_words = (end + 63u) >> 6;                  // <= 165
            const bool last_trip = i0 + kTripToks >= c1;
            const bool keep_last = (end & 63u) != 0u && !last_trip;     // the last word is unfinished and this wave goes on
            const uint32_t n_out = keep_last ? n_words - 1u : n_words;
            unsigned long long kept = 0;
            for (uint32_t w = (uint32_t)lane; w < n_words; w += 64u) {
                const unsigned long long val = stage[w];
                stage[w] = 0ull;
                if (w >= n_out) {
                    kept = val;                 // one lane
                    continue;
                }
                unsigned long long *dst = words[k] + (first >> 6) + w;
                const bool shared = (w == 0u && i0 == c0) || (w == n_words - 1u && last_trip);
                if (shared)
                    atomicOr(dst, val);
                else
                    *dst = val;
            }
            if (keep_last) {
                const uint32_t src = (n_words - 1u) & 63u;
                carry[k] = (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)kept, (int)src) |
                           (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(kept >> 32), (int)src) << 32;
            }
            else {
                carry[k] = 0ull;
            }
            base[k] = first + total;
        }
    }
    // trailers: the Adler-32 of the raster's tile, big endian, after the last (padded) byte
    if ((uint32_t)t < nj && ((coded >> t) & 1u)) {
        const uint32_t j = j0 + (uint32_t)t;
        const Book *b = reinterpret_cast<const Book *>(job.t.books + ((size_t)j * tiles + tix) * kBookBytes);
        const uint32_t adler = job.t.hist[((size_t)j * tiles + tix) * kHistWords + 290];
        uint32_t *w = reinterpret_cast<uint32_t *>(job.t.arena + sh.slot[t]);
        const uint32_t at = b->stream_bytes - 4u;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            const uint32_t byte = (adler >> (24 - 8 * i)) & 0xffu;
            atomicOr(&w[(at + i) >> 2], byte << (8 * ((at + i) & 3u)));
        }
    }
    if (stored_mask == 0)
        return;

    // stored fallback (incompressible tiles): the raster's bytes are val(class), two blocks of
    // 32768 bytes; the classes are formed again from landcover + soil
    __syncthreads();
    for (int i = t; i < gcn10::kClassCodes * 256 / 4; i += kTile)
        reinterpret_cast<uint32_t *>(sh.class_of)[i] = reinterpret_cast<const uint32_t *>(job.class_of)[i];
    __syncthreads();
    for (uint32_t k = 0; k < nj; k++) {
        if (!((stored_mask >> k) & 1u))
            continue;
        const uint32_t j = j0 + k;
        uint8_t *o = job.t.arena + sh.slot[k];
        const uint32_t adler = job.t.hist[((size_t)j * tiles + tix) * kHistWords + 290];
        if (t == 0) {
            o[0] = 0x78;
            o[1] = 0x01;
            for (int blk = 0; blk < 2; blk++) {
                uint8_t *h = o + 2 + blk * (5 + 32768);
                h[0] = (uint8_t)(blk == 1);
                h[1] = 0x00;
                h[2] = 0x80;
                h[3] = 0xff;
                h[4] = 0x7f;
            }
            const uint32_t at = (uint32_t)kMaxStream - 4u;
            o[at] = (uint8_t)(adler >> 24);
            o[at + 1] = (uint8_t)(adler >> 16);
            o[at + 2] = (uint8_t)(adler >> 8);
            o[at + 3] = (uint8_t)adler;
        }
        const uint8_t *val = class_val + job.sel[j] * 256;
        const uint32_t xc = (uint32_t)(t & 63) * 4u;
        for (int i = 0; i < kTile / 4; i++) {
            const int r = i * 4 + (t >> 6);
            const uint32_t c4 = class_pixels4(job, tx * kTile + xc, ty * kTile + (uint32_t)r, sh.class_of);
            uint8_t *dst = o + 2 + (r >> 7) * (5 + 32768) + 5 + (r & 127) * kTile + xc;
            dst[0] = val[c4 & 0xffu];
            dst[1] = val[(c4 >> 8) & 0xffu];
            dst[2] = val[(c4 >> 16) & 0xffu];
            dst[3] = val[c4 >> 24];
        }
    }
}

// Pass F-C for every (tile position, group of rasters) of the job, in the form opt.fused_emit names.
int launch_fused_emit(gcn10_gpu_ctx *ctx, const FusedJob &job, hipStream_t s)
{
    static_assert(sizeof(SharedFC) <= 20 * 1024, "eight fused emit workgroups per CU");
    static_assert(sizeof(SharedFC2) <= 16 * 1024, "ten wave-independent emit workgroups per CU by LDS");
    if (!ctx->fused_emit_ready) {
        HIP_TRY(gcn10::allow_dynamic_lds(fused_emit_wave_kernel, sizeof(SharedFC2)));
        HIP_TRY(gcn10::allow_dynamic_lds(fused_emit_kernel, sizeof(SharedFC)));
        ctx->fused_emit_ready = true;
    }
    const dim3 grid(job.t.across * job.t.down, (job.n_sel + kGroup - 1) / kGroup);
    if (ctx->opt.fused_emit == 0)
        hipLaunchKernelGGL(fused_emit_kernel, grid, dim3(kTile), sizeof(SharedFC), s, job);
    else
        hipLaunchKernelGGL(fused_emit_wave_kernel, grid, dim3(kTile), sizeof(SharedFC2), s, job);
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}

}  // namespace

#endif
