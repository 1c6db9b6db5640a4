// gcn10_lzw_decode.hip -- TIFF LZW decoding of landcover tiles on the GPU (GCN10_TILE_LZW tiles of
// gcn10_gpu_inflate_tiles).
//
// What it is for: `gdal_translate -co COMPRESS=LZW` is how most users repack or clip the landcover, and the
// program's own compress=lzw output is LZW too.  Without this kernel such windows went through the host
// reader (tiff_codec.c lzw_decode on the I/O pool) and 1.3 GB of decoded pixels per 36000^2 block crossed PCIe.
// Here the compressed chunks cross, as for DEFLATE, and are decoded into the same linear scratch slots
// inflate_kernel uses, so untile_kernel does the window copy and the predictor-2 sum-back unchanged
// (gcn10_inflate_internal.hpp: what a tile's flags, status, slot and wanted bytes are for the three kernels).
//
// Semantics are those of tiff_codec.c lzw_decode, exactly: MSB-first codes of 9..12 bits with the "early change"
// of the width, ClearCode 256, EndOfInformation 257, KwKwK (code == next), a dictionary that stops growing
// at 4096 entries (codes stay 12 bits until a Clear), codes after out_len bytes are padding, output past
// out_len is cut, an early EOI leaves zeros in the rest of the chunk.  Errors (status): a code beyond the
// dictionary (GCN10_INFLATE_E_LZW_CODE), a first code after a Clear -- or at the start -- that is not a
// literal (E_LZW_FIRST), input that ends without EOI before out_len bytes (E_LZW_INPUT).  (KwKwK with a
// full dictionary cannot occur: codes have at most 12 bits, so code == next <= 4095.)
//
// Design: LZW as LZ77.  The entry made by the n-th code after a Clear (n >= 1) is the string of code n-1
// plus one byte -- and that string already lies in the output: it starts where code n-1's string was
// written, D[n-1], and is D[n] - D[n-1] + 1 bytes long.  So the dictionary is one array of output
// positions, start[n] = D[n] (15 KiB of LDS), and every code is a copy from earlier output.
//   batch    one wave per stream; between Clears the width of a code depends only on its index, so lane l
//            reads code n0 + l at a bit offset it computes on its own (the input is held in registers, one
//            dword per lane of a 256-byte window, read with bpermute).  The batch ends at the first Clear,
//            EOI, error or missing code (a ballot).
//   lengths  a literal is 1 byte; an entry made before the batch has its length in LDS; an entry made
//            inside the batch is one byte longer than the code before the one that made it -- pointer
//            jumping over the lanes resolves those chains in at most six rounds.  A wave scan of the
//            lengths gives every code's output position.
//   copy     the batch's output is written 64 bytes per step, one byte per lane: a lane finds its code
//            (prefix max over marks of where codes start), then its source byte -- a literal, the last
//            4 KiB of output in an LDS ring, or older output in the tile's slot in HBM.  A source inside
//            the same 64-byte step (short codes, KwKwK runs) is resolved by pointer jumping between lanes.
//            A KwKwK code's last byte is its own first byte: its source is the start of the entry.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): 19.5 KiB of LDS per stream (8 streams
// per CU, a block's 1296 tiles in one round of 2048 slots), 1 wave per workgroup, 38 VGPRs, 77 SGPRs,
// no scratch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gcn10_gpu.h"
#include "gcn10_inflate_internal.hpp"

namespace {

constexpr uint32_t kRing = 4096;            // recent output in LDS
constexpr uint32_t kRingMask = kRing - 1u;
constexpr uint32_t kStarts = 3839;          // start[0..3838]: entries 258..4095 need D[0..3838]
constexpr uint32_t kLit = 0x80000000u;      // source word of a literal: kLit | byte

struct LzwShared {
    uint32_t start[kStarts];                // D[n], output position of the n-th code after the last Clear
    uint8_t mark[64];                       // step-local: which code starts at byte w + i (255 = none)
    uint8_t ring[kRing];                    // output position p at ring[p & kRingMask]
};

// bits of codes 0..n-1 after a Clear: code n is 9 bits wide while n < 254, 10 while n < 766, 11 while n < 1790
// (next = 257 + n reaches 511, 1023, 2047: the early change), then 12
__device__ __forceinline__ unsigned long long bits_before(uint32_t n)
{
    unsigned long long b = 9ull * n;
    b += n > 254u ? n - 254u : 0u;
    b += n > 766u ? n - 766u : 0u;
    b += n > 1790u ? n - 1790u : 0u;
    return b;
}

__device__ __forceinline__ uint32_t width_of(uint32_t n)
{
    return n < 254u ? 9u : n < 766u ? 10u : n < 1790u ? 11u : 12u;
}

__device__ __forceinline__ uint32_t in_dword(const uint32_t *in, uint32_t n_dwords, uint32_t d)
{
    return d < n_dwords ? in[d] : 0u;
}

// LDS accesses of one wave are carried out in order; this keeps the compiler from moving them across phases
__device__ __forceinline__ void wave_lds_order()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(64) void lzw_decode_kernel(const uint8_t *comp, const gcn10_inflate_tile *tiles,
                                                        uint32_t n_tiles, uint8_t *scratch, uint32_t slot_bytes,
                                                        uint32_t *status)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    LzwShared &sh = *reinterpret_cast<LzwShared *>(smem);
    const uint32_t lane = threadIdx.x;
    const uint32_t tile = blockIdx.x;
    if (tile >= n_tiles)
        return;
    const gcn10_inflate_tile tin = tiles[tile];
    if (!(tin.flags & GCN10_TILE_LZW))
        return;                                 // inflate_kernel's
    if (tin.flags & GCN10_TILE_RAW) {
        if (lane == 0)
            status[tile] = GCN10_INFLATE_E_HEADER;
        return;
    }
    if (!gcn10::inflate_window_ok(tin.out_len, tin.chunk_w, tin.src_x, tin.src_y, tin.copy_w, tin.copy_h, slot_bytes)) {
        if (lane == 0)
            status[tile] = GCN10_INFLATE_E_WINDOW;
        return;
    }
    uint8_t *out = scratch + (size_t)tile * slot_bytes;
    const uint32_t cap = tin.out_len < slot_bytes ? tin.out_len : slot_bytes;  // (an empty window passes any out_len)
    const uint32_t *in = reinterpret_cast<const uint32_t *>(comp + tin.in_off);
    const uint32_t n_dwords = (tin.in_len + 3u) / 4u;
    const unsigned long long in_bits = 8ull * tin.in_len;

    // input window: lane l holds dword base + l (in_a) and base + 64 + l (in_b); a batch reads at most
    // 64 * 12 bits = 24 dwords past its first, and starts within the first 32 dwords of the window
    uint32_t base = 0;
    uint32_t in_a = in_dword(in, n_dwords, lane), in_b = in_dword(in, n_dwords, 64u + lane);

    unsigned long long bitpos = 0;  // of code n0
    uint32_t n0 = 0;                // codes since the last Clear (or the start)
    uint32_t op = 0;                // output position (may pass cap on the last code)
    uint32_t err = 0;
    bool done = cap == 0;           // (the host reader returns at once for an empty chunk)
    while (!done) {
        if ((uint32_t)(bitpos >> 5) - base >= 32u) {
            base += 32u;
            const uint32_t a_hi = (uint32_t)__shfl((int)in_a, (int)((lane + 32u) & 63u));
            const uint32_t b_lo = (uint32_t)__shfl((int)in_b, (int)((lane + 32u) & 63u));
            in_a = lane < 32u ? a_hi : b_lo;
            in_b = lane < 32u ? b_lo : in_dword(in, n_dwords, base + 64u + lane);
        }
        // ---- lane l: code n0 + l
        const uint32_t n = n0 + lane;
        const uint32_t wd = width_of(n);
        const unsigned long long bp = bitpos + (bits_before(n) - bits_before(n0));
        const bool exists = bp + wd <= in_bits;
        uint32_t code;
        {
            uint32_t rel = (uint32_t)(bp >> 5) - base;
            rel = exists && rel < 63u ? rel : 62u;
            const uint32_t hi = __builtin_bswap32((uint32_t)__shfl((int)in_a, (int)rel));
            const uint32_t lo = __builtin_bswap32((uint32_t)__shfl((int)in_a, (int)rel + 1));
            const unsigned long long x = (unsigned long long)hi << 32 | lo;
            code = (uint32_t)((x << (bp & 31u)) >> (64u - wd));
        }
        const uint32_t next = n == 0u ? 258u : (257u + n < 4096u ? 257u + n : 4096u);   // before code n
        const bool special = !exists || code == 256u || code == 257u || (n == 0u ? code >= 256u : code > next);
        const unsigned long long sp_mask = __ballot(special);
        uint32_t cnt = sp_mask ? (uint32_t)__builtin_ctzll(sp_mask) : 64u;
        const bool active = lane < cnt;

        // ---- lengths and sources
        uint32_t len = 0, src = 0, ref = 64u;   // ref: lane whose output position is the source
        bool res = true;
        if (active) {
            if (code < 256u) {
                len = 1u;
                src = kLit | code;
            } else {
                const uint32_t m = code - 258u;   // entry m: D[m], D[m+1] - D[m] + 1 bytes
                if (m + 1u < n0) {
                    src = sh.start[m];
                    len = sh.start[m + 1u] - src + 1u;
                } else if (m + 1u == n0) {
                    src = sh.start[m];
                    len = op - src + 1u;
                } else {
                    ref = m - n0;                 // < lane
                    len = 1u;
                    res = false;
                }
            }
        }
        {
            // len(lane) = len + len(ptr) while unresolved: pointer jumping
            uint32_t ptr = res ? lane : ref;
            while (__ballot(!res)) {
                const uint32_t p_len = (uint32_t)__shfl((int)len, (int)ptr);
                const uint32_t p_ptr = (uint32_t)__shfl((int)ptr, (int)ptr);
                const bool p_res = __shfl((int)res, (int)ptr) != 0;
                if (!res) {
                    len += p_len;
                    if (p_res)
                        res = true;
                    else
                        ptr = p_ptr;
                }
            }
        }
        uint32_t incl = len;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, off, 64);
            if ((int)lane >= off)
                incl += up;
        }
        const uint32_t D = op + incl - len;
        {
            const uint32_t rsrc = (uint32_t)__shfl((int)D, (int)(ref & 63u));
            if (ref < 64u)
                src = rsrc;
        }
        // the code that reaches out_len is the last one
        const unsigned long long full = __ballot(active && D + len >= cap);
        bool finished = false;
        if (full) {
            cnt = (uint32_t)__builtin_ctzll(full) + 1u;
            finished = true;
        }
        const uint32_t total = (uint32_t)__shfl((int)incl, (int)(cnt ? cnt - 1u : 0u)) * (cnt ? 1u : 0u);
        if (lane < cnt && n < kStarts)
            sh.start[n] = D;
        wave_lds_order();

        // ---- copy, 64 bytes per step
        const uint32_t emit_end = op + total < cap ? op + total : cap;
        uint32_t cur = 0;                       // the code that holds the step's first byte
        for (uint32_t w = op; w < emit_end; w += 64u) {
            sh.mark[lane] = 255u;
            wave_lds_order();
            if (lane < cnt && D >= w && D < w + 64u)
                sh.mark[D - w] = (uint8_t)lane;
            wave_lds_order();
            int c = sh.mark[lane];
            c = c == 255 ? (int)cur : c;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int up = __shfl_up(c, off, 64);
                if ((int)lane >= off && up > c)
                    c = up;
            }
            cur = (uint32_t)__shfl(c, 63);
            const uint32_t q = w + lane;
            const bool valid = q < emit_end;
            const uint32_t cD = (uint32_t)__shfl((int)D, c);
            const uint32_t cS = (uint32_t)__shfl((int)src, c);
            uint32_t v = 0, ptr = lane;
            bool known = true, far = false;
            uint32_t s = 0;
            if (valid) {
                if (cS & kLit) {
                    v = cS & 0xffu;
                } else {
                    s = cS + (q - cD);
                    if (s >= cD)
                        s = cS;                 // KwKwK: the last byte is the entry's first
                    if (s >= w) {
                        ptr = s - w;
                        known = false;
                    } else if (w - s <= kRing) {
                        v = sh.ring[s & kRingMask];
                    } else {
                        far = true;
                    }
                }
            }
            if (__ballot(far)) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's stores of the slot are done
                if (far)
                    v = out[s];
            }
            while (__ballot(!known)) {
                const uint32_t p_v = (uint32_t)__shfl((int)v, (int)ptr);
                const uint32_t p_ptr = (uint32_t)__shfl((int)ptr, (int)ptr);
                const bool p_known = __shfl((int)known, (int)ptr) != 0;
                if (!known) {
                    if (p_known) {
                        v = p_v;
                        known = true;
                    } else {
                        ptr = p_ptr;
                    }
                }
            }
            wave_lds_order();
            if (valid) {
                sh.ring[q & kRingMask] = (uint8_t)v;
                out[q] = (uint8_t)v;
            }
            wave_lds_order();
        }
        op += total;
        if (finished)
            break;
        // ---- what ended the batch
        if (cnt == 64u) {
            bitpos += bits_before(n0 + 64u) - bits_before(n0);
            n0 += 64u;
            continue;
        }
        const uint32_t sp_code = (uint32_t)__shfl((int)code, (int)cnt);
        const bool sp_exists = __shfl((int)exists, (int)cnt) != 0;
        if (!sp_exists) {
            err = GCN10_INFLATE_E_LZW_INPUT;    // input ended without EOI before out_len bytes
            break;
        }
        if (sp_code == 257u)
            break;                              // EOI
        if (sp_code == 256u) {                  // Clear
            bitpos += bits_before(n0 + cnt) - bits_before(n0) + width_of(n0 + cnt);
            n0 = 0;
            continue;
        }
        err = n0 + cnt == 0u ? GCN10_INFLATE_E_LZW_FIRST : GCN10_INFLATE_E_LZW_CODE;
        break;
    }
    // zeros up to the chunk's size (an early EOI; as the host reader and the DEFLATE path leave it)
    for (uint32_t i = (op < cap ? op : cap) + lane; i < cap; i += 64u)
        out[i] = 0;
    if (lane == 0)
        status[tile] = err;
}

}  // namespace

namespace gcn10 {

void launch_lzw_decode(const uint8_t *comp_dev, const gcn10_inflate_tile *tiles_dev, uint32_t n_tiles,
                       uint8_t *scratch, uint32_t slot_bytes, uint32_t *status_dev, hipStream_t stream)
{
    static_assert(sizeof(LzwShared) <= 20 * 1024, "eight streams per CU of 160 KiB LDS");
    hipLaunchKernelGGL(lzw_decode_kernel, dim3(n_tiles), dim3(64), sizeof(LzwShared), stream, comp_dev, tiles_dev,
                       n_tiles, scratch, slot_bytes, status_dev);
}

}  // namespace gcn10
