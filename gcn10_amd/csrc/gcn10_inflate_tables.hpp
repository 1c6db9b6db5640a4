// gcn10_inflate_tables.hpp -- the bit reader and the canonical-code tables of the DEFLATE decoder.  Included by
// gcn10_inflate.hip alone, inside its anonymous namespace (the file says why the pieces are headers).
//   input    each decoder lane holds one dword of a 256-byte piece of the stream (plus the next piece, already in
//            flight, and the one before); the bit reader takes dwords with v_readlane at a wave-uniform index, so the
//            decode state lives in scalar registers
//   tables   canonical codes are sorted by (length, symbol) with ballots; the 10-bit (literal/length) and 9-bit
//            (distance) lookup tables are filled entry-parallel, 16 resp. 8 entries per lane; longer codes take a
//            bit-serial canonical walk (slow_symbol)
#ifndef GCN10_INFLATE_TABLES_HPP
#define GCN10_INFLATE_TABLES_HPP

struct Reader {
    const uint32_t *in;     // 16-byte aligned start of the stream
    uint32_t n_dwords;      // dwords that hold stream bytes
    uint32_t ip;            // next dword to take
    uint32_t chunk;         // index of the 64-dword piece held in `cur`
    uint32_t cur, nxt;      // per lane
    uint32_t prv;           // per lane: the piece before `cur` (the bit buffer may still hold bits of it)
    unsigned long long bb;  // bit buffer, LSB first
    uint32_t bc;            // valid bits in bb
    int lane;
};

__device__ __forceinline__ uint32_t load_piece(const Reader &r, uint32_t chunk)
{
    const uint32_t i = chunk * 64u + (uint32_t)r.lane;
    return i < r.n_dwords ? r.in[i] : 0u;
}

__device__ __forceinline__ void reader_seek(Reader &r, uint32_t dword)
{
    r.ip = dword;
    r.chunk = dword >> 6;
    r.cur = load_piece(r, r.chunk);
    r.nxt = load_piece(r, r.chunk + 1);
    r.prv = 0;
    r.bb = 0;
    r.bc = 0;
}

// The stream is held a piece (64 dwords, one per lane) at a time: the piece before the
// current one, the current one and the next (already in flight).  Pieces only ever advance.
__device__ __forceinline__ void ensure_piece(Reader &r, uint32_t c)
{
    if (c == r.chunk + 1u) {                    // wave-uniform
        r.prv = r.cur;
        r.cur = r.nxt;
        r.chunk = c;
        r.nxt = load_piece(r, c + 1);
    }
}

// dword q of the stream as a wave-uniform value (q lies in one of the three pieces)
__device__ __forceinline__ uint32_t stream_dword(const Reader &r, uint32_t q)
{
    const uint32_t in_prv = (uint32_t)__builtin_amdgcn_readlane((int)r.prv, (int)(q & 63u));
    const uint32_t in_cur = (uint32_t)__builtin_amdgcn_readlane((int)r.cur, (int)(q & 63u));
    const uint32_t in_nxt = (uint32_t)__builtin_amdgcn_readlane((int)r.nxt, (int)(q & 63u));
    const uint32_t c = q >> 6;
    return c == r.chunk ? in_cur : (c + 1u == r.chunk ? in_prv : in_nxt);
}

__device__ __forceinline__ uint32_t take_dword(Reader &r)
{
    ensure_piece(r, r.ip >> 6);
    const uint32_t v = stream_dword(r, r.ip);
    r.ip++;
    return v;
}

// at least 33 bits in the buffer afterwards
__device__ __forceinline__ void refill(Reader &r)
{
    if (r.bc <= 32) {
        r.bb |= (unsigned long long)take_dword(r) << r.bc;
        r.bc += 32;
    }
}

__device__ __forceinline__ uint32_t take_bits(Reader &r, uint32_t n)
{
    const uint32_t v = (uint32_t)r.bb & ((1u << n) - 1u);
    r.bb >>= n;
    r.bc -= n;
    return v;
}

// bytes of the stream consumed so far (whole bytes only)
__device__ __forceinline__ uint32_t reader_byte_pos(const Reader &r)
{
    return r.ip * 4u - r.bc / 8u;
}

// the scalar reader at bit P of the stream (P lies in the current piece or the one before)
__device__ __forceinline__ void seek_bits(Reader &r, uint32_t P)
{
    r.ip = P >> 5;
    r.bb = 0;
    r.bc = 0;
    refill(r);
    take_bits(r, P & 31u);
}

struct Code {               // canonical code, by length
    uint16_t count[16];
    uint16_t first[16];     // first code of each length
    uint16_t offs[16];      // index of its symbol in sorted[]
};

// Sorts the n symbols of lens[] by (length, symbol) and derives first code / offset per
// length.  Returns false for a set zlib refuses (inftrees.c): lengths that over-subscribe the code
// space, or an incomplete code -- which zlib allows only for a code with no symbol at all or with a
// single 1-bit code, and for the precode (`precode`) only with no symbol at all.
__device__ __forceinline__ bool sort_code(const uint8_t *lens, int n, uint16_t *sorted, Code &c, int lane,
                                          bool precode = false)
{
    uint32_t cnt[16];
#pragma unroll
    for (int L = 0; L < 16; L++)
        cnt[L] = 0;
    for (int base = 0; base < n; base += 64) {
        const int s = base + lane;
        const uint32_t mylen = s < n ? lens[s] : 0u;
#pragma unroll
        for (int L = 1; L < 16; L++)
            cnt[L] += (uint32_t)__builtin_popcountll(__ballot(mylen == (uint32_t)L));
    }
    uint32_t offs[16], first[16];
    int left = 1, longest = 0;
    bool ok = true;
    offs[0] = 0;
    first[0] = 0;
    offs[1] = 0;
    first[1] = 0;
#pragma unroll
    for (int L = 1; L < 16; L++) {
        left = left * 2 - (int)cnt[L];
        if (left < 0)
            ok = false;
        if (cnt[L] != 0)
            longest = L;
        if (L < 15) {
            offs[L + 1] = offs[L] + cnt[L];
            first[L + 1] = (first[L] + cnt[L]) << 1;
        }
    }
    if (left > 0 && longest != 0 && (precode || longest != 1))
        ok = false;                     // incomplete
    if (lane < 16) {
        uint32_t cv = 0, fv = 0, ov = 0;
#pragma unroll
        for (int L = 1; L < 16; L++) {
            if (lane == L) {
                cv = cnt[L];
                fv = first[L];
                ov = offs[L];
            }
        }
        c.count[lane] = (uint16_t)cv;
        c.first[lane] = (uint16_t)fv;
        c.offs[lane] = (uint16_t)ov;
    }
    uint32_t run[16];
#pragma unroll
    for (int L = 0; L < 16; L++)
        run[L] = offs[L];
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int base = 0; base < n; base += 64) {
        const int s = base + lane;
        const uint32_t mylen = s < n ? lens[s] : 0u;
#pragma unroll
        for (int L = 1; L < 16; L++) {
            const unsigned long long m = __ballot(mylen == (uint32_t)L);
            if (mylen == (uint32_t)L)
                sorted[run[L] + (uint32_t)__builtin_popcountll(m & below)] = (uint16_t)s;
            run[L] += (uint32_t)__builtin_popcountll(m);
        }
    }
    return ok;
}

// Table entries, indexed by the low ROOT bits of the bit buffer (codes arrive MSB first, so
// the buffer's bit 0 is a code's first bit).  Bits 0..3 of an entry = bits to consume, 0 = no
// code of at most ROOT bits starts here (longer code, or none).
//   literal/length table   bits 4..5 kind: 0 literals, 1 match length, 2 end of block
//     literals  bits 6..7 how many (1..3: as many whole literal codes as fit the ROOT bits),
//               bits 8..31 their bytes, first one lowest
//     length    bits 6..8 number of extra bits, bits 9..17 base length
//   distance table         bits 4..7 number of extra bits, bits 8..23 base distance
//   code-length table      bits 4..8 symbol
enum { kLiterals = 0, kLength = 1, kEndOfBlock = 2 };

__device__ __forceinline__ uint32_t length_entry(uint32_t sym, uint32_t bits)
{
    // sym = 257..285, RFC 1951 3.2.5
    const uint32_t s = sym - 257u;
    if (s > 28u)
        return 0;
    uint32_t base, eb = 0;
    if (s < 8u) {
        base = 3u + s;
    }
    else if (s == 28u) {
        base = 258u;
    }
    else {
        eb = (s - 4u) >> 2;
        base = 3u + ((4u + (s & 3u)) << eb);
    }
    return bits | (uint32_t)kLength << 4 | eb << 6 | base << 9;
}

__device__ __forceinline__ uint32_t dist_entry(uint32_t sym, uint32_t bits)
{
    if (sym > 29u)
        return 0;
    uint32_t base, eb = 0;
    if (sym < 4u) {
        base = 1u + sym;
    }
    else {
        eb = (sym - 2u) >> 1;
        base = 1u + ((2u + (sym & 1u)) << eb);
    }
    return bits | eb << 4 | base << 8;
}

// the code at the low bits of `v`, looking at no more than `avail` (<= ROOT) of them:
// symbol << 4 | length, or 0
template <int ROOT>
__device__ __forceinline__ uint32_t walk(uint32_t v, int avail, const uint32_t (&cnt)[ROOT + 1],
                                         const uint32_t (&first)[ROOT + 1], const uint32_t (&offs)[ROOT + 1],
                                         const uint16_t *sorted)
{
    uint32_t code = 0, e = 0;
#pragma unroll
    for (int L = 1; L <= ROOT; L++) {
        code = (code << 1) | ((v >> (L - 1)) & 1u);
        const uint32_t d = code - first[L];
        if (e == 0 && L <= avail && code >= first[L] && d < cnt[L])
            e = (uint32_t)sorted[offs[L] + d] << 4 | (uint32_t)L;
    }
    return e;
}

enum { kCodeLengthTable = 0, kLitLenTable = 1, kDistTable = 2 };

template <int ROOT, int WHICH>
__device__ __forceinline__ void fill_table(uint32_t *tab, const uint16_t *sorted, const Code &c, int lane)
{
    uint32_t cnt[ROOT + 1], first[ROOT + 1], offs[ROOT + 1];
#pragma unroll
    for (int L = 1; L <= ROOT; L++) {
        cnt[L] = c.count[L];
        first[L] = c.first[L];
        offs[L] = c.offs[L];
    }
    for (int idx = lane; idx < (1 << ROOT); idx += 64) {
        const uint32_t w = walk<ROOT>((uint32_t)idx, ROOT, cnt, first, offs, sorted);
        uint32_t e = 0;
        if (w != 0) {
            const uint32_t sym = w >> 4, bits = w & 15u;
            if (WHICH == kCodeLengthTable) {
                e = w;
            }
            else if (WHICH == kDistTable) {
                e = dist_entry(sym, bits);
            }
            else if (sym == 256u) {
                e = bits | (uint32_t)kEndOfBlock << 4;
            }
            else if (sym > 256u) {
                e = length_entry(sym, bits);
            }
            else {
                // up to three literals whose codes fit the ROOT bits together
                uint32_t bytes = sym, n = 1, used = bits;
#pragma unroll
                for (int more = 0; more < 2; more++) {
                    const uint32_t w2 = used < (uint32_t)ROOT && n == (uint32_t)more + 1u
                                            ? walk<ROOT>((uint32_t)idx >> used, ROOT - (int)used, cnt, first, offs, sorted)
                                            : 0u;
                    if (w2 != 0 && (w2 >> 4) < 256u) {
                        bytes |= (w2 >> 4) << (8 * n);
                        n++;
                        used += w2 & 15u;
                    }
                }
                e = used | (uint32_t)kLiterals << 4 | n << 6 | bytes << 8;
            }
        }
        tab[idx] = e;
    }
}

// a code longer than the table's root, or none: walk the canonical code bit by bit;
// symbol << 4 | length, or 0
__device__ __forceinline__ uint32_t slow_symbol(const Reader &r, const uint16_t *sorted, const Code &c)
{
    uint32_t code = 0;
    for (int L = 1; L < 16; L++) {
        code = (code << 1) | ((uint32_t)(r.bb >> (L - 1)) & 1u);
        const uint32_t f = c.first[L], n = c.count[L];
        if (code >= f && code - f < n)
            return (uint32_t)sorted[c.offs[L] + code - f] << 4 | (uint32_t)L;
    }
    return 0;
}

#endif
