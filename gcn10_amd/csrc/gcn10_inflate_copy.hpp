// gcn10_inflate_copy.hpp -- the COPIER wave of the DEFLATE decoder: token words carried out on the LDS ring, finished
// flush units sent to HBM.  Included by gcn10_inflate.hip alone, inside its anonymous namespace, behind the constants,
// Shared and gcn10_inflate_decode.hpp (the token words).  copy_batch takes a batch of literals and matches in
// sub-batches of at most kSubCap bytes, five stages each; copy_batch_serial takes a batch that holds a stored run token
// by token; copy_match is one match by all 64 lanes, whatever its shape; copy_long the long match of stage B2.
#ifndef GCN10_INFLATE_COPY_HPP
#define GCN10_INFLATE_COPY_HPP

struct Output {
    uint8_t *out;           // this tile's slot in HBM, 16-byte aligned -- or, for a tile decoded in place, the first
                            // byte of its window in the destination raster
    uint32_t limit;         // bytes wanted
    uint32_t pos;           // bytes produced
    uint32_t flushed;       // bytes already in HBM (multiple of kFlush)
    // A tile decoded IN PLACE (round 3): the whole chunk is wanted, it is a power of two wide and its rows start on
    // 16-byte boundaries of the destination, so decoded byte p goes straight to row p / width, column p % width of the
    // raster -- no slot, no pass of untile_kernel over it (94 % of a block's tiles: all but its last row and column).
    uint32_t wshift;        // log2(chunk width); 0 = the linear slot
    uint32_t wmask;
    unsigned long long stride;
};

__device__ __forceinline__ uint8_t *out_at(const Output &o, uint32_t p)
{
    return o.wshift ? o.out + (size_t)(p >> o.wshift) * o.stride + (p & o.wmask) : o.out + p;
}

__device__ __forceinline__ void flush_half(Shared &sh, Output &o, int lane)
{
    const u32x4 *src = reinterpret_cast<const u32x4 *>(sh.window + (o.flushed & kWindowMask));
#pragma unroll 4
    for (int i = lane; i < kFlush / 16; i += 64)
        *reinterpret_cast<u32x4 *>(out_at(o, o.flushed + 16u * (uint32_t)i)) = src[i];      // (16 bytes never leave a row: widths are multiples of 16)
    o.flushed += kFlush;
}

// `ahead`: bytes of the ring from this token's first byte up to the furthest byte already written (the
// token's own length when tokens are carried out strictly in order; more when later tokens of the
// sub-batch have been carried out first): the ring bytes that far behind have been overwritten.
__device__ __forceinline__ void copy_match(Shared &sh, Output &o, uint32_t len, uint32_t dist, uint32_t ahead, int lane)
{
    const uint32_t from = o.pos - dist;
    if (dist + ahead > (uint32_t)kWindow) {
        // the source starts before what the ring still holds: all of it has been flushed to the slot
        // (from + len < flushed + kFlush + kSubCap - kWindow + len <= flushed: a sub-batch starts with fewer than
        // kFlush bytes pending and ends at most kSubCap further, and kFlush + kSubCap + 258 <= kWindow)
        // -- wait for those stores, read it back
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        uint8_t v[5];
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const uint32_t k = (uint32_t)lane + 64u * (uint32_t)i;
            v[i] = k < len ? *out_at(o, from + k) : (uint8_t)0;
        }
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const uint32_t k = (uint32_t)lane + 64u * (uint32_t)i;
            if (k < len)
                sh.window[(o.pos + k) & kWindowMask] = v[i];
        }
    }
    else if (len <= 64u && dist >= len) {
        // the usual case: one step, source and destination apart
        if ((uint32_t)lane < len)
            sh.window[(o.pos + (uint32_t)lane) & kWindowMask] = sh.window[(from + (uint32_t)lane) & kWindowMask];
    }
    else if (dist >= len) {
        // source and destination apart, up to 258 bytes: all the reads first, then all the writes
        // (one LDS round trip instead of five)
        uint8_t v[5];
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const uint32_t k = (uint32_t)lane + 64u * (uint32_t)i;
            v[i] = k < len ? sh.window[(from + k) & kWindowMask] : (uint8_t)0;
        }
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const uint32_t k = (uint32_t)lane + 64u * (uint32_t)i;
            if (k < len)
                sh.window[(o.pos + k) & kWindowMask] = v[i];
        }
    }
    else if (dist >= 64u) {
        // 64 bytes per step; a later step may read what an earlier one wrote (LDS keeps order)
        for (uint32_t base = 0; base < len; base += 64u) {
            const uint32_t k = base + (uint32_t)lane;
            if (k < len)
                sh.window[(o.pos + k) & kWindowMask] = sh.window[(from + k) & kWindowMask];
        }
    }
    else if (dist == 1u && len >= 16u && (o.pos & (uint32_t)kWindowMask) + len <= (uint32_t)kWindow) {
        // a long run of one byte (every constant stretch of a landcover row is one), not across the ring's end: the
        // byte four times in a dword, one dword per lane and up to three bytes behind them.  (Runs of a few bytes,
        // which i.i.d. pixels are full of, stay with the general form below: it is faster for them.)
        const uint32_t d_off = o.pos & (uint32_t)kWindowMask;
        const uint32_t v = (uint32_t)sh.window[from & kWindowMask] * 0x01010101u;
        const uint32_t n4 = len >> 2, r = len & 3u;
        typedef uint32_t u32_u __attribute__((aligned(1)));
        if ((uint32_t)lane < n4)
            *reinterpret_cast<u32_u *>(sh.window + d_off + 4u * (uint32_t)lane) = v;
        if ((uint32_t)lane < r)
            sh.window[d_off + 4u * n4 + (uint32_t)lane] = (uint8_t)v;
    }
    else {
        // the copy repeats the last `dist` bytes: lane l always writes pattern byte l mod dist
        // when the step is a multiple of dist
        uint32_t step = dist;
        while (step * 2u <= 64u)
            step *= 2u;
        const uint32_t q = (uint32_t)(((float)lane + 0.5f) * __builtin_amdgcn_rcpf((float)dist));
        const uint8_t v = sh.window[(from + ((uint32_t)lane - q * dist)) & kWindowMask];
        for (uint32_t base = 0; base < len; base += step) {
            const uint32_t k = base + (uint32_t)lane;
            if ((uint32_t)lane < step && k < len)
                sh.window[(o.pos + k) & kWindowMask] = v;
        }
    }
    o.pos += len;
}

// A match of 65..258 bytes whose source and destination ranges lie apart in the ring and do not cross its end
// (offsets s_off, d_off): one dword per lane (unaligned LDS access is enabled on this platform), one byte per lane
// for the last 0..3 bytes, ONE wait for those two reads, two writes.  copy_match()'s form of the same copy is five
// predicated byte reads and five predicated byte writes, ~100 instructions (cycle counters, round 3: 900 cycles per
// 258-byte match, and a patchy tile's decode waits for its copier).
__device__ __forceinline__ void copy_long(Shared &sh, uint32_t s_off, uint32_t d_off, uint32_t len, int lane)
{
    const uint32_t base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t *)sh.window;
    const uint32_t n4 = len >> 2, r = len & 3u;                 // whole dwords (16..64), bytes behind them
    const unsigned long long m4 = n4 >= 64u ? ~0ull : (1ull << n4) - 1ull, mr = (1ull << r) - 1ull;
    const uint32_t a4 = base + s_off + 4u * (uint32_t)lane, b4 = base + d_off + 4u * (uint32_t)lane;
    const uint32_t a1 = base + s_off + 4u * n4 + (uint32_t)lane, b1 = base + d_off + 4u * n4 + (uint32_t)lane;
    uint32_t v0, v1;
    unsigned long long sv;
    asm volatile("s_mov_b64 %[sv], exec\n\t"
                 "s_mov_b64 exec, %[m4]\n\t"
                 "ds_read_b32 %[v0], %[a4]\n\t"
                 "s_mov_b64 exec, %[mr]\n\t"
                 "ds_read_u8 %[v1], %[a1]\n\t"
                 "s_waitcnt lgkmcnt(0)\n\t"
                 "ds_write_b8 %[b1], %[v1]\n\t"
                 "s_mov_b64 exec, %[m4]\n\t"
                 "ds_write_b32 %[b4], %[v0]\n\t"
                 "s_mov_b64 exec, %[sv]"
                 : [v0] "=&v"(v0), [v1] "=&v"(v1), [sv] "=&s"(sv)
                 : [a4] "v"(a4), [b4] "v"(b4), [a1] "v"(a1), [b1] "v"(b1), [m4] "s"(m4), [mr] "s"(mr)
                 : "memory");
}

// A batch of tokens carried out one by one, in order (batches that hold a stored run).
// Returns 0, or the reason a token cannot be carried out (a distance before the start).
__device__ __forceinline__ uint32_t copy_batch_serial(Shared &sh, Output &o, const uint32_t *ring, uint32_t n,
                                               const uint8_t *stream, int lane)
{
    const uint32_t tk = (uint32_t)lane < n ? ring[lane] : 0u;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)tk, (int)i);
        if (o.pos >= o.limit)
            break;
        if (a & kTokMatch) {
            uint32_t len = ((a >> 16) & 255u) + 3u;
            const uint32_t dist = (a & 0xffffu) + 1u;
            if (dist > o.pos)
                return GCN10_INFLATE_E_DISTANCE;
            if (len > o.limit - o.pos)
                len = o.limit - o.pos;
            copy_match(sh, o, len, dist, len, lane);
        }
        else if (a & kTokStored) {
            const uint32_t len = a & 0xffffu;
            i++;
            const uint32_t at = (uint32_t)__builtin_amdgcn_readlane((int)tk, (int)i);
            for (uint32_t k = lane; k < len; k += 64)
                sh.window[(o.pos + k) & kWindowMask] = stream[at + k];
            o.pos += len;
        }
        else {
            const uint32_t cnt = a >> 24;
            if ((uint32_t)lane < cnt)
                sh.window[(o.pos + (uint32_t)lane) & kWindowMask] = (uint8_t)(a >> (8 * lane));
            o.pos += cnt;
        }
        if (o.pos - o.flushed >= (uint32_t)kFlush)
            flush_half(sh, o, lane);
    }
    return 0;
}

// The copier wave: carries out a batch of tokens on the window and sends finished halves to HBM.
// Returns 0, or the reason a token cannot be carried out (a distance before the start).
//
// One token per lane.  A prefix sum of the tokens' lengths gives every token its place; the batch is
// taken in sub-batches of at most kSubCap bytes (the ring must keep what is not flushed yet), and in
// each sub-batch, in this order,
//   A   all literal tokens write their 1..3 bytes at once.  They read nothing.
//   B   the matches of at most kShortMatch bytes whose source is still in the ring once the whole sub-batch is out
//       (`near`), lies wholly before the sub-batch, and which cross the ring's end with neither range, copy their bytes
//       at once, one lane per match.  Their source was final before the sub-batch began and nothing in it overwrites it.
//   F   the matches of at most 64 bytes whose source has left the ring (not `near`) read it from HBM, eight matches
//       at a time, a lane per byte.  It was flushed before the sub-batch began, so it is final too.
//   B2  the matches of more than kShortMatch bytes that meet B's other conditions, one after the other with every lane
//       at work (copy_long).  Final sources, as in B.
//   C   the remaining matches one by one, in stream order, by all 64 lanes (copy_match): those that read bytes of this
//       sub-batch (their own among them), those with a range across the ring's end, and the long ones out of HBM.
// A token carried out early only writes bytes of its own place, so the order of A, B, F and B2 among tokens that do not
// read each other's output is free; C runs last and in stream order, and by then every byte an earlier token produces
// is there.
__device__ __forceinline__ uint32_t copy_batch(Shared &sh, Output &o, const uint32_t *ring, uint32_t n,
                                               const uint8_t *stream, int lane)
{
    const uint32_t tk = (uint32_t)lane < n ? ring[lane] : 0u;
    const bool valid = (uint32_t)lane < n;
    if (__ballot(valid && !(tk & kTokMatch) && (tk & kTokStored)) != 0ull)
        return copy_batch_serial(sh, o, ring, n, stream, lane);
    const bool is_match = (tk & kTokMatch) != 0u;
    const uint32_t dist = (tk & 0xffffu) + 1u;
    uint32_t done = 0;
    while (done < n && o.pos < o.limit) {
        const bool in = valid && (uint32_t)lane >= done;
        const uint32_t len = !in ? 0u : is_match ? ((tk >> 16) & 255u) + 3u : (tk >> 24);
        const uint32_t incl = wave_scan(len);
        const uint32_t off = incl - len;
        const uint32_t m = (uint32_t)__builtin_popcountll(__ballot(in && incl <= kSubCap));    // >= 1
        const bool mine = in && (uint32_t)lane < done + m;
        const uint32_t S = (uint32_t)__builtin_amdgcn_readlane((int)incl, (int)((done + m - 1u) & 63u));
        const uint32_t dst = o.pos + off;
        // bytes wanted of this token: none behind the limit, the one that reaches it is cut
        uint32_t l = !mine || dst >= o.limit ? 0u : (len < o.limit - dst ? len : o.limit - dst);
        if (__ballot(is_match && l > 0u && dist > dst) != 0ull)
            return GCN10_INFLATE_E_DISTANCE;
        const uint32_t ahead = S - off;                     // ring bytes written from dst on, once the sub-batch is out
        const bool near = dist + ahead <= (uint32_t)kWindow;
        // (stage B copies with unaligned dword accesses that must stay inside the ring: neither range across its end)
        const uint32_t s_ring = (dst - dist) & (uint32_t)kWindowMask, d_ring = dst & (uint32_t)kWindowMask;
        const bool early = is_match && l > 0u && l <= kShortMatch && near && dist >= off + l &&
                           s_ring + l <= (uint32_t)kWindow && d_ring + l <= (uint32_t)kWindow;
        // ... and the longer ones of the same kind (a patchy tile is made of them: 258 bytes from the row above),
        // one after the other but with every lane at work: stage B2
        const bool early_long = is_match && l > kShortMatch && near && dist >= off + l &&
                                s_ring + l <= (uint32_t)kWindow && d_ring + l <= (uint32_t)kWindow;
        // A: literals
        if (!is_match && l > 0u) {
#pragma unroll
            for (uint32_t b = 0; b < 3u; b++)
                if (b < l)
                    sh.window[(dst + b) & kWindowMask] = (uint8_t)(tk >> (8u * b));
        }
        // B: matches of up to kShortMatch bytes that read nothing of this sub-batch, all at once, one lane per match:
        // up to sixteen dword steps (unaligned LDS access is enabled on this platform) and up to three single bytes, all
        // the reads, ONE wait, all the writes.  Written out: the masks are scalar (ballots), the steps differ only in
        // their immediate offsets, and the compiler would wait after every read.  Round 3: this stage took matches
        // of at most 8 bytes, byte by byte; carried out one by one in stage C a match costs ~35 instructions of a
        // wave that shares its SIMD's issue slots with the decoders (profiles/r03/decoder_cycle_counters.txt).
        if (__ballot(early) != 0ull) {
            const uint32_t base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t *)sh.window;
            const uint32_t n4 = early ? l >> 2 : 0u, r = early ? l & 3u : 0u;
            unsigned long long M[16], T[3];
#pragma unroll
            for (uint32_t k = 0; k < 16u; k++)
                M[k] = __ballot(k < n4);
#pragma unroll
            for (uint32_t k = 0; k < 3u; k++)
                T[k] = __ballot(k < r);
            const uint32_t a = base + s_ring, b = base + d_ring, at = a + 4u * n4, bt = b + 4u * n4;
            uint32_t v0, v1, v2, v3, v4, v5, v6, v7, v8, v9, v10, v11, v12, v13, v14, v15, t0, t1, t2;
            unsigned long long sv;
            asm volatile("s_mov_b64 %[sv], exec\n\t"
                         "s_mov_b64 exec, %[M0]\n\t"
                         "ds_read_b32 %[v0], %[a]\n\t"
                         "s_mov_b64 exec, %[M1]\n\t"
                         "ds_read_b32 %[v1], %[a] offset:4\n\t"
                         "s_mov_b64 exec, %[M2]\n\t"
                         "ds_read_b32 %[v2], %[a] offset:8\n\t"
                         "s_mov_b64 exec, %[M3]\n\t"
                         "ds_read_b32 %[v3], %[a] offset:12\n\t"
                         "s_mov_b64 exec, %[M4]\n\t"
                         "ds_read_b32 %[v4], %[a] offset:16\n\t"
                         "s_mov_b64 exec, %[M5]\n\t"
                         "ds_read_b32 %[v5], %[a] offset:20\n\t"
                         "s_mov_b64 exec, %[M6]\n\t"
                         "ds_read_b32 %[v6], %[a] offset:24\n\t"
                         "s_mov_b64 exec, %[M7]\n\t"
                         "ds_read_b32 %[v7], %[a] offset:28\n\t"
                         "s_mov_b64 exec, %[M8]\n\t"
                         "ds_read_b32 %[v8], %[a] offset:32\n\t"
                         "s_mov_b64 exec, %[M9]\n\t"
                         "ds_read_b32 %[v9], %[a] offset:36\n\t"
                         "s_mov_b64 exec, %[M10]\n\t"
                         "ds_read_b32 %[v10], %[a] offset:40\n\t"
                         "s_mov_b64 exec, %[M11]\n\t"
                         "ds_read_b32 %[v11], %[a] offset:44\n\t"
                         "s_mov_b64 exec, %[M12]\n\t"
                         "ds_read_b32 %[v12], %[a] offset:48\n\t"
                         "s_mov_b64 exec, %[M13]\n\t"
                         "ds_read_b32 %[v13], %[a] offset:52\n\t"
                         "s_mov_b64 exec, %[M14]\n\t"
                         "ds_read_b32 %[v14], %[a] offset:56\n\t"
                         "s_mov_b64 exec, %[M15]\n\t"
                         "ds_read_b32 %[v15], %[a] offset:60\n\t"
                         "s_mov_b64 exec, %[T0]\n\t"
                         "ds_read_u8 %[t0], %[at]\n\t"
                         "s_mov_b64 exec, %[T1]\n\t"
                         "ds_read_u8 %[t1], %[at] offset:1\n\t"
                         "s_mov_b64 exec, %[T2]\n\t"
                         "ds_read_u8 %[t2], %[at] offset:2\n\t"
                         "s_waitcnt lgkmcnt(0)\n\t"
                         "ds_write_b8 %[bt], %[t2] offset:2\n\t"
                         "s_mov_b64 exec, %[T1]\n\t"
                         "ds_write_b8 %[bt], %[t1] offset:1\n\t"
                         "s_mov_b64 exec, %[T0]\n\t"
                         "ds_write_b8 %[bt], %[t0]\n\t"
                         "s_mov_b64 exec, %[M15]\n\t"
                         "ds_write_b32 %[b], %[v15] offset:60\n\t"
                         "s_mov_b64 exec, %[M14]\n\t"
                         "ds_write_b32 %[b], %[v14] offset:56\n\t"
                         "s_mov_b64 exec, %[M13]\n\t"
                         "ds_write_b32 %[b], %[v13] offset:52\n\t"
                         "s_mov_b64 exec, %[M12]\n\t"
                         "ds_write_b32 %[b], %[v12] offset:48\n\t"
                         "s_mov_b64 exec, %[M11]\n\t"
                         "ds_write_b32 %[b], %[v11] offset:44\n\t"
                         "s_mov_b64 exec, %[M10]\n\t"
                         "ds_write_b32 %[b], %[v10] offset:40\n\t"
                         "s_mov_b64 exec, %[M9]\n\t"
                         "ds_write_b32 %[b], %[v9] offset:36\n\t"
                         "s_mov_b64 exec, %[M8]\n\t"
                         "ds_write_b32 %[b], %[v8] offset:32\n\t"
                         "s_mov_b64 exec, %[M7]\n\t"
                         "ds_write_b32 %[b], %[v7] offset:28\n\t"
                         "s_mov_b64 exec, %[M6]\n\t"
                         "ds_write_b32 %[b], %[v6] offset:24\n\t"
                         "s_mov_b64 exec, %[M5]\n\t"
                         "ds_write_b32 %[b], %[v5] offset:20\n\t"
                         "s_mov_b64 exec, %[M4]\n\t"
                         "ds_write_b32 %[b], %[v4] offset:16\n\t"
                         "s_mov_b64 exec, %[M3]\n\t"
                         "ds_write_b32 %[b], %[v3] offset:12\n\t"
                         "s_mov_b64 exec, %[M2]\n\t"
                         "ds_write_b32 %[b], %[v2] offset:8\n\t"
                         "s_mov_b64 exec, %[M1]\n\t"
                         "ds_write_b32 %[b], %[v1] offset:4\n\t"
                         "s_mov_b64 exec, %[M0]\n\t"
                         "ds_write_b32 %[b], %[v0]\n\t"
                         "s_mov_b64 exec, %[sv]"
                         : [v0] "=&v"(v0), [v1] "=&v"(v1), [v2] "=&v"(v2), [v3] "=&v"(v3), [v4] "=&v"(v4), [v5] "=&v"(v5), [v6] "=&v"(v6), [v7] "=&v"(v7), [v8] "=&v"(v8), [v9] "=&v"(v9), [v10] "=&v"(v10), [v11] "=&v"(v11), [v12] "=&v"(v12), [v13] "=&v"(v13), [v14] "=&v"(v14), [v15] "=&v"(v15), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [sv] "=&s"(sv)
                         : [a] "v"(a), [b] "v"(b), [at] "v"(at), [bt] "v"(bt), [M0] "s"(M[0]), [M1] "s"(M[1]), [M2] "s"(M[2]), [M3] "s"(M[3]), [M4] "s"(M[4]), [M5] "s"(M[5]), [M6] "s"(M[6]), [M7] "s"(M[7]), [M8] "s"(M[8]), [M9] "s"(M[9]), [M10] "s"(M[10]), [M11] "s"(M[11]), [M12] "s"(M[12]), [M13] "s"(M[13]), [M14] "s"(M[14]), [M15] "s"(M[15]), [T0] "s"(T[0]), [T1] "s"(T[1]), [T2] "s"(T[2])
                         : "memory");
        }
        // F: matches whose source has left the ring (it lies in the tile's slot in HBM, flushed: copy_match()) and that
        // are at most 64 bytes long, eight at a time: eight byte loads per lane in flight, one wait, eight LDS writes.
        // One by one in stage C each was a memory round trip of its own behind a wait for all stores -- a noisy tile has
        // 5 700 of them with the 8 KiB ring, a third of what was left of the copier's time (decoder_cycle_counters.txt).
        // Their sources are final, they write only their own place: any time before the stages that may read them.
        const bool far_short = is_match && l > 0u && l <= 64u && !near;
        {
            unsigned long long todo = __ballot(far_short);
            if (todo != 0ull)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the flushes this wave has issued are in the slot
            while (todo != 0ull) {
                uint32_t f_dst[8], f_l[8];
                uint8_t v[8];
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    f_l[k] = 0;
                    f_dst[k] = 0;
                    v[k] = 0;
                    if (todo != 0ull) {
                        const int i = __builtin_ctzll(todo);
                        todo &= todo - 1ull;
                        f_dst[k] = (uint32_t)__builtin_amdgcn_readlane((int)dst, i);
                        f_l[k] = (uint32_t)__builtin_amdgcn_readlane((int)l, i);
                        const uint32_t from = f_dst[k] - (uint32_t)__builtin_amdgcn_readlane((int)dist, i);
                        if ((uint32_t)lane < f_l[k])
                            v[k] = *out_at(o, from + (uint32_t)lane);
                    }
                }
#pragma unroll
                for (int k = 0; k < 8; k++)
                    if ((uint32_t)lane < f_l[k])
                        sh.window[(f_dst[k] + (uint32_t)lane) & kWindowMask] = v[k];
            }
        }
        // B2: long matches that read nothing of this sub-batch
        for (unsigned long long todo = __ballot(early_long); todo != 0ull; todo &= todo - 1ull) {
            const int i = __builtin_ctzll(todo);
            copy_long(sh, (uint32_t)__builtin_amdgcn_readlane((int)s_ring, i), (uint32_t)__builtin_amdgcn_readlane((int)d_ring, i),
                      (uint32_t)__builtin_amdgcn_readlane((int)l, i), lane);
        }
        // C: the other matches, in order
        unsigned long long rest = __ballot(is_match && l > 0u && !early && !early_long && !far_short);
        const uint32_t pos0 = o.pos;
        while (rest != 0ull) {
            const int i = __builtin_ctzll(rest);
            rest &= rest - 1ull;
            o.pos = (uint32_t)__builtin_amdgcn_readlane((int)dst, i);
            copy_match(sh, o, (uint32_t)__builtin_amdgcn_readlane((int)l, i),
                       (uint32_t)__builtin_amdgcn_readlane((int)dist, i),
                       (uint32_t)__builtin_amdgcn_readlane((int)ahead, i), lane);
        }
        o.pos = pos0 + S < o.limit ? pos0 + S : o.limit;
        done += m;
        if (o.pos - o.flushed >= (uint32_t)kFlush)
            flush_half(sh, o, lane);
    }
    return 0;
}

#endif
