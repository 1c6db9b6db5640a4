// gcn10_inflate_decode.hpp -- the DECODER wave of the DEFLATE decoder: bits into token words, kBatch at a time.
// Included by gcn10_inflate.hip alone, inside its anonymous namespace, behind the constants, Shared and
// gcn10_inflate_tables.hpp.  begin_block reads a block header and builds its tables, decode_batch fills one half of
// the token ring (speculative lanes and the scalar chain walk inside a block), scalar_token takes the one token whose
// code the tables do not hold.  Malformed streams end with d.err = GCN10_INFLATE_E_* and d.state = kDone.
#ifndef GCN10_INFLATE_DECODE_HPP
#define GCN10_INFLATE_DECODE_HPP

// Tokens the decoder wave hands to the copier wave, one word each (a stored run takes two):
//   literals  how many (1..3) << 24 | their bytes, first one lowest
//   match     0x80000000 | (length - 3) << 16 | (distance - 1)
//   stored    0x40000000 | length (<= kSubCap), then a word with the offset of the bytes in the stream
constexpr uint32_t kTokMatch = 0x80000000u, kTokStored = 0x40000000u;

enum { kNeedHeader = 0, kInSymbols = 1, kInStored = 2, kDone = 3 };

struct Decoder {            // the decoder wave's state between batches (all wave-uniform)
    Reader r;
    uint32_t state;
    uint32_t P;             // kInSymbols: bit position in the stream (the reader's own bit state is stale)
    uint32_t pos, limit;    // bytes the tokens so far produce; bytes wanted
    uint32_t stored_left, stored_at;
    uint32_t err;
    bool last;              // the current block is the final one
    uint32_t in_len;
};

// Parses a block header (and builds its tables).  Leaves d.state = kInSymbols / kInStored, or
// kDone with d.err set.
__device__ __forceinline__ void begin_block(Shared &sh, Decoder &d, int lane)
{
    Reader &r = d.r;
    refill(r);
    d.last = take_bits(r, 1) != 0;
    const uint32_t type = take_bits(r, 2);
    if (type == 0) {
        // stored: skip to the byte boundary, LEN, NLEN, LEN bytes
        take_bits(r, r.bc & 7u);
        refill(r);
        const uint32_t len = take_bits(r, 16);
        refill(r);
        const uint32_t nlen = take_bits(r, 16);
        if ((len ^ nlen) != 0xffffu) {
            d.err = GCN10_INFLATE_E_STORED;
            d.state = kDone;
            return;
        }
        d.stored_at = reader_byte_pos(r);
        d.stored_left = len;
        if (d.stored_at + len > d.in_len) {
            d.err = GCN10_INFLATE_E_INPUT;
            d.state = kDone;
            return;
        }
        d.state = kInStored;
        return;
    }
    if (type == 3) {
        d.err = GCN10_INFLATE_E_BLOCK_TYPE;
        d.state = kDone;
        return;
    }
    int n_lit, n_dist;
    if (type == 1) {
        // fixed code: lengths 8 / 9 / 7 / 8, 30 distance codes of 5 bits (RFC 1951 3.2.6)
        for (int i = lane; i < 288; i += 64)
            sh.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
        if (lane < 32)
            sh.lens[288 + lane] = 5;
        n_lit = 288;
        n_dist = 32;
    }
    else {
        n_lit = (int)take_bits(r, 5) + 257;
        n_dist = (int)take_bits(r, 5) + 1;
        const int n_cl = (int)take_bits(r, 4) + 4;
        if (n_lit > 286 || n_dist > 30) {
            d.err = GCN10_INFLATE_E_LENGTHS;
            d.state = kDone;
            return;
        }
        // code-length code: 19 symbols of up to 7 bits, table over 7 bits in lit_tab
        if (lane < 19)
            sh.lens[lane] = 0;
        for (int i = 0; i < n_cl; i++) {
            refill(r);
            const uint32_t v = take_bits(r, 3);
            // i: 0 1 2 3 | 4 5 6 7 8 9 10 11 12 13 14 15 16 17 18 -> 16 17 18 0 | 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
            const int sym = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? (19 - i) / 2 : 8 + (i - 4) / 2;
            if (lane == 0)
                sh.lens[sym] = (uint8_t)v;
        }
        if (!sort_code(sh.lens, 19, sh.lit_sorted, sh.lit, lane, true)) {
            d.err = GCN10_INFLATE_E_LENGTHS;
            d.state = kDone;
            return;
        }
        fill_table<7, kCodeLengthTable>(sh.lit_tab, sh.lit_sorted, sh.lit, lane);
        // the n_lit + n_dist code lengths, run-length coded
        int have = 0;
        uint32_t prev = 0;
        const int total = n_lit + n_dist;
        while (have < total) {
            refill(r);
            const uint32_t e = uniform(sh.lit_tab[(uint32_t)r.bb & 127u]);
            if (e == 0) {
                d.err = GCN10_INFLATE_E_LENGTHS;
                break;
            }
            take_bits(r, e & 15u);
            const uint32_t sym = e >> 4;
            uint32_t rep = 1, val = sym;
            if (sym == 16) {
                if (have == 0) {
                    d.err = GCN10_INFLATE_E_LENGTHS;
                    break;
                }
                rep = 3 + take_bits(r, 2);
                val = prev;
            }
            else if (sym == 17) {
                rep = 3 + take_bits(r, 3);
                val = 0;
            }
            else if (sym == 18) {
                rep = 11 + take_bits(r, 7);
                val = 0;
            }
            if (have + (int)rep > total) {
                d.err = GCN10_INFLATE_E_LENGTHS;
                break;
            }
            for (uint32_t k = lane; k < rep; k += 64)
                sh.lens[have + k] = (uint8_t)val;       // lens[] is re-used: the 19 are in the table now
            have += (int)rep;
            prev = val;
        }
        if (d.err) {
            d.state = kDone;
            return;
        }
        // distance lengths follow the literal/length ones: move them to lens[288..]
        {
            const uint8_t dl = lane < n_dist ? sh.lens[n_lit + lane] : (uint8_t)0;
            if (lane < 32)
                sh.lens[288 + lane] = dl;
            for (int i = n_lit + lane; i < 288; i += 64)
                sh.lens[i] = 0;
        }
        if (uniform(sh.lens[256]) == 0u) {      // no end-of-block code: zlib refuses the block
            d.err = GCN10_INFLATE_E_LENGTHS;
            d.state = kDone;
            return;
        }
        n_lit = 288;
        n_dist = 32;
    }
    if (!sort_code(sh.lens, n_lit, sh.lit_sorted, sh.lit, lane) ||
        !sort_code(sh.lens + 288, n_dist, sh.dist_sorted, sh.dist, lane)) {
        d.err = GCN10_INFLATE_E_LENGTHS;
        d.state = kDone;
        return;
    }
    fill_table<kLitRoot, kLitLenTable>(sh.lit_tab, sh.lit_sorted, sh.lit, lane);
    fill_table<kDistRoot, kDistTable>(sh.dist_tab, sh.dist_sorted, sh.dist, lane);
    d.P = r.ip * 32u - r.bc;
    d.state = kInSymbols;
}

// One token by the scalar bit reader (codes longer than the tables' roots, or none).  The reader
// must stand at the token.  Returns false when the block or the stream ends here.
__device__ __forceinline__ bool scalar_token(Shared &sh, Decoder &d, uint32_t *ring, uint32_t &n, int lane)
{
    Reader &r = d.r;
    refill(r);
    uint32_t e = uniform(sh.lit_tab[(uint32_t)r.bb & ((1u << kLitRoot) - 1u)]);
    if (e == 0) {
        const uint32_t w = uniform(slow_symbol(r, sh.lit_sorted, sh.lit));
        const uint32_t sym = w >> 4;
        e = w == 0        ? 0u
            : sym < 256u  ? ((w & 15u) | 1u << 6 | sym << 8)
            : sym == 256u ? ((w & 15u) | (uint32_t)kEndOfBlock << 4)
                          : length_entry(sym, w & 15u);
        if (e == 0) {
            d.err = GCN10_INFLATE_E_CODE;
            d.state = kDone;
            return false;
        }
    }
    take_bits(r, e & 15u);
    const uint32_t kind = (e >> 4) & 3u;
    uint32_t tok, outl;
    if (kind == (uint32_t)kLiterals) {
        outl = (e >> 6) & 3u;
        tok = outl << 24 | (e >> 8);
    }
    else if (kind == (uint32_t)kLength) {
        const uint32_t len = ((e >> 9) & 511u) + take_bits(r, (e >> 6) & 7u);
        refill(r);
        uint32_t de = uniform(sh.dist_tab[(uint32_t)r.bb & ((1u << kDistRoot) - 1u)]);
        if (de == 0) {
            const uint32_t w = uniform(slow_symbol(r, sh.dist_sorted, sh.dist));
            de = w == 0 ? 0u : dist_entry(w >> 4, w & 15u);
            if (de == 0) {
                d.err = GCN10_INFLATE_E_CODE;
                d.state = kDone;
                return false;
            }
        }
        take_bits(r, de & 15u);
        const uint32_t dist = ((de >> 8) & 0xffffu) + take_bits(r, (de >> 4) & 15u);
        outl = len;
        tok = kTokMatch | (len - 3u) << 16 | (dist - 1u);
    }
    else {
        d.state = kNeedHeader;                      // end of block
        return false;
    }
    if (lane == 0)
        ring[n] = tok;
    n++;
    d.pos += outl;
    if (d.pos >= d.limit) {
        d.state = kDone;
        return false;
    }
    return true;
}

// The decoder wave: up to kBatch token words into `ring`; returns how many.  Every token
// produces output and output is bounded, every header consumes input and input is bounded, so
// the stream ends (d.state = kDone) whatever its bits are.
//
// Inside a block the 64 lanes decode SPECULATIVELY: lane k decodes the tokens that would start at
// bits P + k, P + 64 + k, ... of a 256-bit window (table lookups as gathers, all in vector
// registers; 8 bits of result per candidate, packed four to a register), and a scalar walk then follows
// the real chain -- start at lane 0, jump by each token's bit count -- collecting the tokens it
// passes.  The serial part of the decode is that walk: one v_readlane and a few scalar
// instructions per token instead of two dependent table lookups.
__device__ __forceinline__ uint32_t decode_batch(Shared &sh, Decoder &d, uint32_t *ring, int lane)
{
    Reader &r = d.r;
    uint32_t n = 0;
    while (n < (uint32_t)kBatch && d.state != (uint32_t)kDone) {
        if (d.state == (uint32_t)kNeedHeader) {
            if (d.last || d.pos >= d.limit) {
                d.state = kDone;
                break;
            }
            begin_block(sh, d, lane);
            continue;
        }
        if (d.state == (uint32_t)kInStored) {
            if (n + 2u > (uint32_t)kBatch)
                break;
            uint32_t len = d.stored_left < kSubCap ? d.stored_left : kSubCap;
            if (len > d.limit - d.pos)
                len = d.limit - d.pos;
            if (len > 0) {
                if (lane == 0) {
                    ring[n] = kTokStored | len;
                    ring[n + 1] = d.stored_at;
                }
                n += 2;
                d.pos += len;
            }
            d.stored_at += len;
            d.stored_left -= len;
            if (d.stored_left == 0 || d.pos >= d.limit) {
                const uint32_t at = d.stored_at + d.stored_left;
                reader_seek(r, at >> 2);
                refill(r);
                take_bits(r, (at & 3u) * 8u);
                d.state = d.pos >= d.limit ? (uint32_t)kDone : (uint32_t)kNeedHeader;
            }
            continue;
        }
        // ---- kInSymbols: one window of 256 candidate start bits at d.P, four per lane ----
        const uint32_t q0 = d.P >> 5;
        ensure_piece(r, q0 >> 6);
        uint32_t D[11];
        if ((q0 & 63u) <= 53u) {
            // the usual case: all eleven dwords in one piece, one select for all of them
            const uint32_t piece = (q0 >> 6) == r.chunk ? r.cur : r.prv;
            const int l0 = (int)(q0 & 63u);
#pragma unroll
            for (int i = 0; i < 11; i++)
                D[i] = (uint32_t)__builtin_amdgcn_readlane((int)piece, l0 + i);
        }
        else {
#pragma unroll
            for (int i = 0; i < 11; i++)
                D[i] = stream_dword(r, q0 + (uint32_t)i);
        }
        const uint32_t rel = (d.P & 31u) + (uint32_t)lane;          // < 95
        const uint32_t o = rel >> 5, sft = rel & 31u;
        uint32_t tok[kCand];
        uint32_t packed = 0;        // per candidate 8 bits: bits it takes (< 64) | stop reason << 6
#pragma unroll
        for (int h = 0; h < kCand; h++) {
            // candidate at bit lane + 64 * h: dwords o + 2 * h .. + 2 of the eleven
            const uint32_t a = o == 0 ? D[2 * h] : o == 1 ? D[2 * h + 1] : D[2 * h + 2];
            const uint32_t b = o == 0 ? D[2 * h + 1] : o == 1 ? D[2 * h + 2] : D[2 * h + 3];
            const uint32_t c = o == 0 ? D[2 * h + 2] : o == 1 ? D[2 * h + 3] : D[2 * h + 4];
            const uint32_t lo = __builtin_amdgcn_alignbit(b, a, sft);   // bits of the candidate .. +31
            const uint32_t hi = __builtin_amdgcn_alignbit(c, b, sft);   //                     +32 .. +63
            const uint32_t e1 = sh.lit_tab[lo & ((1u << kLitRoot) - 1u)];
            const uint32_t cl = e1 & 15u, kind = (e1 >> 4) & 3u;
            uint32_t bits = cl;
            uint32_t tk = ((e1 >> 6) & 3u) << 24 | (e1 >> 8);
            uint32_t special = e1 == 0 ? 2u : (kind == (uint32_t)kEndOfBlock ? 1u : 0u);
            {
                // as if it were a match (harmless where it is not: the lookups stay in the tables)
                const uint32_t eb = (e1 >> 6) & 7u;
                const uint32_t len = ((e1 >> 9) & 511u) + ((lo >> cl) & ((1u << eb) - 1u));
                const uint32_t t = cl + eb;                             // <= 20
                const uint32_t x2 = __builtin_amdgcn_alignbit(hi, lo, t);
                const uint32_t de = sh.dist_tab[x2 & ((1u << kDistRoot) - 1u)];
                const uint32_t dl = de & 15u, deb = (de >> 4) & 15u;
                const uint32_t dist = ((de >> 8) & 0xffffu) + ((x2 >> dl) & ((1u << deb) - 1u));
                if (kind == (uint32_t)kLength && e1 != 0) {
                    bits = t + dl + deb;                                // <= 48
                    tk = kTokMatch | ((len - 3u) & 255u) << 16 | ((dist - 1u) & 0xffffu);
                    if (de == 0)
                        special = 2u;
                }
            }
            // a token the walk passes: its bits; one it stops at: an end of block (with its bits,
            // which the walk takes) or a code the tables do not hold (no bits: the scalar reader
            // starts at it)
            const uint32_t inf8 = special == 2u ? 0x80u : special == 1u ? (cl | 0x40u) : bits;
            packed |= inf8 << (8 * h);
            tok[h] = tk;
        }
        // ---- the chain: from bit 0 of the window, token by token.  One exit, no branches in the
        // body, one v_readlane per token: the loop is the serial core of the decoder.  The bytes the
        // tokens produce are summed afterwards (they are in the token words) ----
        // Written out, 17 instructions per token (the compiler's form of the same loop takes 24): the
        // start bit of the it-th token goes to lane `it` with one v_writelane (lane select in M0: two
        // different SGPR operands would break the constant-bus rule), and the three reasons to stop -- a
        // stop token, the end of the window, a full batch -- are chained through two scalar selects.
        const uint32_t room = (uint32_t)kBatch - n;        // 1..64: also keeps `it` within the 64 lanes
        uint32_t k = 0, it = 0, inf, t0, t1, m0_saved;
        uint32_t src = 0;
        asm volatile("s_mov_b32 %[m0s], m0\n"
                     "1:\n\t"
                     "v_readlane_b32 %[t0], %[packed], %[k]\n\t"       // lane k mod 64
                     "s_lshr_b32 %[t1], %[k], 3\n\t"
                     "s_and_b32 %[t1], %[t1], 24\n\t"
                     "s_mov_b32 m0, %[it]\n\t"
                     "s_lshr_b32 %[t0], %[t0], %[t1]\n\t"
                     "s_and_b32 %[inf], %[t0], 0xff\n\t"
                     "v_writelane_b32 %[src], %[k], m0\n\t"            // src[lane it] = k
                     "s_add_u32 %[it], %[it], 1\n\t"
                     "s_and_b32 %[t0], %[inf], 63\n\t"
                     "s_add_u32 %[k], %[k], %[t0]\n\t"
                     "s_cmp_lt_u32 %[inf], 64\n\t"
                     "s_cselect_b32 %[t0], %[k], 0x100\n\t"            // a stop token ends the walk
                     "s_cmp_lt_u32 %[t0], 0x100\n\t"
                     "s_cselect_b32 %[t0], %[it], %[room]\n\t"         // so does the end of the window
                     "s_cmp_lt_u32 %[t0], %[room]\n\t"                 // ... and a full batch
                     "s_cbranch_scc1 1b\n\t"
                     "s_mov_b32 m0, %[m0s]"                              // (M0 is the compiler's: put it back)
                     : [k] "+s"(k), [it] "+s"(it), [inf] "=&s"(inf), [t0] "=&s"(t0), [t1] "=&s"(t1), [src] "+v"(src),
                       [m0s] "=&s"(m0_saved)
                     : [packed] "v"(packed), [room] "s"(room)
                     : "scc");
        static_assert(kCand == 4, "the walk's window end is written as 0x100");
        uint32_t stop = inf >> 6;
        const uint32_t last_bits = inf & 63u;
        uint32_t n_new = stop != 0u ? it - 1u : it;        // a stop token is not a token of the stream
        {
            const int sel = (int)((src & 63u) << 2);
            uint32_t mine = 0;
#pragma unroll
            for (int h = 0; h < kCand; h++) {
                const uint32_t m = (uint32_t)__builtin_amdgcn_ds_bpermute(sel, (int)tok[h]);
                mine = (src >> 6) == (uint32_t)h ? m : mine;
            }
            const bool kept = (uint32_t)lane < n_new;
            if (kept)
                ring[n + (uint32_t)lane] = mine;
            // bytes of the kept tokens: a match says its length, literals their count
            const uint32_t outl = !kept ? 0u : (mine & kTokMatch) ? ((mine >> 16) & 255u) + 3u : (mine >> 24);
            const uint32_t total = wave_total(outl);
            if (d.pos + total >= d.limit) {
                // the tile ends inside this window (once per stream): keep the tokens up to the one
                // that reaches the limit and stand behind it, exactly -- nothing behind it counts, not
                // even the end-of-block code the walk may have taken
                const uint32_t cum = wave_scan(outl);
                const uint32_t before = (uint32_t)__builtin_popcountll(__ballot(kept && d.pos + cum < d.limit));
                const uint32_t keep = before + 1u < n_new ? before + 1u : n_new;
                const uint32_t k_next = (uint32_t)__builtin_amdgcn_readlane((int)src, (int)(keep & 63u));
                k = keep < n_new ? k_next : (stop == 1u ? k - last_bits : k);
                d.pos += (uint32_t)__builtin_amdgcn_readlane((int)cum, (int)((keep - 1u) & 63u));
                n_new = keep;
                stop = 4u;
            }
            else {
                d.pos += total;
            }
            n += n_new;
        }
        d.P += k;
        if (stop == 4u) {
            d.state = kDone;
        }
        else if (stop == 1u) {
            // end of block (its code is taken): the next header is read by the scalar reader
            seek_bits(r, d.P);
            d.state = kNeedHeader;
        }
        else if (stop == 2u) {
            // a code the tables do not hold (or none): that one token by the scalar reader
            if (n < (uint32_t)kBatch) {
                seek_bits(r, d.P);
                if (scalar_token(sh, d, ring, n, lane) || d.state == (uint32_t)kNeedHeader)
                    d.P = r.ip * 32u - r.bc;
            }
            else {
                break;                              // no room: the next batch starts with it
            }
        }
        if (d.state == (uint32_t)kDone)
            seek_bits(r, d.P);                      // (for the end-of-input check)
    }
    return n;
}

#endif
