// gcn10_arena_place.hip -- the arena / table / cursor contract of the three tile encoders (gcn10_deflate.hip,
// gcn10_deflate_fused.hip, gcn10_lzw.hip), codec-neutral: the checks of the arguments every entry point takes and
// the tile grid of a strip (tile_job_setup), the worst-case arena (arena_bound), and pass B', the kernel that lays
// the finished sizes out as one extent per raster.  gcn10_amd/gpu.py has the same contract once, on the Python side
// (Engine._encode_into_arena).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gcn10_deflate_internal.hpp"
#include "gcn10_gpu.h"
#include "gcn10_gpu_internal.hpp"

using gcn10::fail;
using namespace gcn10_deflate;

namespace {

// ------------------------------------------------------------------------
// pass B': where every stream goes.  One workgroup; streams are laid out in index order
// (raster-major, tiles of a raster row-major), 16-byte aligned, and every raster's first
// stream starts at a multiple of `seg_align`: the streams of one raster of a strip are ONE
// contiguous extent of the arena, in tile order, so the host appends them to the raster's
// GeoTIFF with a single write (and, with seg_align = 4096, may do so with O_DIRECT straight
// from the pinned copy of the arena).  Replaces the atomic slot reservation of rounds 1-2,
// whose order was the order in which the code-construction waves happened to finish.
// Aliases (fused encoder: this raster's tile is another raster's stream) take no room.
// *cursor = arena bytes used, pads included; a stream that does not fit gets offset
// 0xffffffff and size 0, as before.
// ------------------------------------------------------------------------
constexpr int kPlaceThreads = 1024;

// Pass B left table[i] = { alias mark or 0, stream bytes }: 8 contiguous bytes per stream, so a thread's
// K consecutive entries are a few cache lines (the first form of this kernel read the sizes out of the
// 1.1 KB code books: 54 us per strip; this one: a few us).
__device__ __forceinline__ uint32_t place_need(uint32_t mark, uint32_t bytes)
{
    return mark == kAliasSlot ? 0u : (bytes + (uint32_t)(kSlotAlign - 1)) & ~(uint32_t)(kSlotAlign - 1);
}

__device__ __forceinline__ unsigned long long seg_of_pad(const unsigned long long (&sg)[GCN10_N_RASTERS + 1], uint32_t r)
{
    unsigned long long v = 0;
#pragma unroll
    for (uint32_t q = 0; q <= (uint32_t)GCN10_N_RASTERS; q++)
        v = q == r ? sg[q] : v;
    return v;
}

__global__ __launch_bounds__(kPlaceThreads) void deflate_place_kernel(const TileJob job, uint32_t tiles_per_raster,
                                                                      uint32_t seg_align)
{
    __shared__ unsigned long long wave_tot[kPlaceThreads / 64];
    __shared__ unsigned long long P[GCN10_N_RASTERS + 1];       // unaligned prefix at each raster's first stream
    __shared__ unsigned long long seg[GCN10_N_RASTERS + 1];     // where each raster's extent starts
    constexpr uint32_t kMaxK = 40;                              // entries per thread kept in registers (40 960 streams)
    const uint32_t t = threadIdx.x;
    const uint32_t n = job.n_tiles;
    const uint32_t n_rasters = n / tiles_per_raster;
    const uint32_t K = (n + kPlaceThreads - 1) / kPlaceThreads;
    const uint32_t i0 = t * K < n ? t * K : n, i1 = i0 + K < n ? i0 + K : n;
    const uint2 *tab = reinterpret_cast<const uint2 *>(job.table);

    // one pass over the table: the thread's entries stay in registers (K <= kMaxK: strips of up to 4 096 rows of a
    // 36000-px block; larger launches re-read), its sum, and its sum up to the raster boundary it may contain
    // (K < tiles_per_raster whenever a raster has more tiles than a thread has entries: at most one boundary)
    uint32_t need[kMaxK];
    unsigned long long sum = 0, sum_at_boundary = 0;
    uint32_t boundary = 0xffffffffu;                            // the raster that starts inside this thread's range
    const bool in_regs = K <= kMaxK && K < tiles_per_raster;
    if (in_regs) {
#pragma unroll
        for (uint32_t k = 0; k < kMaxK; k++) {
            need[k] = 0;
            if (k < K && i0 + k < i1) {
                const uint2 e = tab[i0 + k];
                need[k] = place_need(e.x, e.y) | (e.x == kAliasSlot ? 0x80000000u : 0u);
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < kMaxK; k++)
            if (k < K && i0 + k < i1) {
                if ((i0 + k) % tiles_per_raster == 0) {
                    boundary = (i0 + k) / tiles_per_raster;
                    sum_at_boundary = sum;
                }
                sum += need[k] & 0x7fffffffu;
            }
    }
    else {
        for (uint32_t i = i0; i < i1; i++) {
            const uint2 e = tab[i];
            sum += place_need(e.x, e.y);
        }
    }
    // exclusive scan over the workgroup
    unsigned long long incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long up = __shfl_up(incl, off, 64);
        if ((int)(t & 63u) >= off)
            incl += up;
    }
    if ((t & 63u) == 63u)
        wave_tot[t >> 6] = incl;
    __syncthreads();
    unsigned long long base = incl - sum, total = 0;
    for (uint32_t w = 0; w < kPlaceThreads / 64; w++) {
        if (w < (t >> 6))
            base += wave_tot[w];
        total += wave_tot[w];
    }
    if (in_regs) {
        if (boundary != 0xffffffffu)
            P[boundary] = base + sum_at_boundary;
    }
    else {
        unsigned long long running = base;
        for (uint32_t i = i0; i < i1; i++) {
            const uint2 e = tab[i];
            if (i % tiles_per_raster == 0)
                P[i / tiles_per_raster] = running;
            running += place_need(e.x, e.y);
        }
    }
    if (t == 0)
        P[n_rasters] = total;
    __syncthreads();
    // every thread works the extents out for itself (18 steps on LDS values: cheaper than a third barrier)
    unsigned long long my_seg[GCN10_N_RASTERS + 1];
    {
        const unsigned long long a = seg_align;
        my_seg[0] = 0;
#pragma unroll
        for (uint32_t r = 1; r <= (uint32_t)GCN10_N_RASTERS; r++) {
            const unsigned long long end = r <= n_rasters ? my_seg[r - 1] + (P[r] - P[r - 1]) : 0ull;
            my_seg[r] = r < n_rasters ? (end + a - 1) / a * a : end;
        }
        if (t == 0) {
            unsigned long long used = 0;
#pragma unroll
            for (uint32_t r = 0; r <= (uint32_t)GCN10_N_RASTERS; r++) {
                seg[r] = my_seg[r];
                used = r == n_rasters ? my_seg[r] : used;
            }
            *job.cursor = used;
        }
    }
    {
        unsigned long long running = base;
        const uint32_t r0 = i0 < n ? i0 / tiles_per_raster : 0u;
        auto seg_of = [&](uint32_t r) -> unsigned long long {
            unsigned long long v = 0;
#pragma unroll
            for (uint32_t q = 0; q <= (uint32_t)GCN10_N_RASTERS; q++)
                v = q == r ? my_seg[q] : v;
            return v;
        };
        if (in_regs) {
            // (at most two rasters in a thread's range)
            const unsigned long long sa = seg_of(r0), pa = P[r0 < n_rasters ? r0 : 0], sb = seg_of(r0 + 1),
                                     pb = P[r0 + 1 <= n_rasters ? r0 + 1 : 0];
#pragma unroll
            for (uint32_t k = 0; k < kMaxK; k++)
                if (k < K && i0 + k < i1) {
                    const uint32_t i = i0 + k;
                    const bool second = i / tiles_per_raster != r0;
                    const uint32_t nd = need[k] & 0x7fffffffu;
                    if (!(need[k] & 0x80000000u)) {
                        const unsigned long long off = (second ? sb : sa) + (running - (second ? pb : pa));
                        const bool fits = off + nd <= job.arena_cap;
                        job.table[(size_t)i * 2] = fits ? (uint32_t)off : 0xffffffffu;
                        if (!fits)
                            job.table[(size_t)i * 2 + 1] = 0u;
                    }
                    running += nd;
                }
        }
        else {
            for (uint32_t i = i0; i < i1; i++) {
                const uint2 e = tab[i];
                const uint32_t r = i / tiles_per_raster;
                const uint32_t nd = place_need(e.x, e.y);
                if (e.x != kAliasSlot) {
                    const unsigned long long off = seg_of(r) + (running - P[r]);
                    const bool fits = off + nd <= job.arena_cap;
                    job.table[(size_t)i * 2] = fits ? (uint32_t)off : 0xffffffffu;
                    if (!fits)
                        job.table[(size_t)i * 2 + 1] = 0u;
                }
                running += nd;
            }
        }
    }
    // the pad between a raster's last stream and the next raster's extent reads as zeros, and so do the
    // bytes from the last stream's end to the next multiple of the alignment (an O_DIRECT write reads them):
    // wave w zeroes behind rasters w, w + 16
    for (uint32_t r = t >> 6; r < n_rasters; r += kPlaceThreads / 64) {
        const unsigned long long from = seg_of_pad(my_seg, r) + (P[r + 1] - P[r]);
        unsigned long long to = r + 1 < n_rasters ? seg_of_pad(my_seg, r + 1) : (from + seg_align - 1) / seg_align * seg_align;
        if (to > job.arena_cap)
            to = job.arena_cap;
        for (unsigned long long o = from + (unsigned long long)(t & 63u) * 16u; o + 16u <= to; o += 64u * 16u)
            *reinterpret_cast<gcn10::u32x4 *>(job.arena + o) = gcn10::u32x4{ 0u, 0u, 0u, 0u };
    }
}

}  // namespace

namespace gcn10 {

int tile_job_setup(const char *who, int W, int rows, int streams, uint8_t *arena, size_t arena_cap, uint32_t *table,
                   unsigned long long *cursor, TileJob *job)
{
    *job = TileJob{};
    if (streams < 1 || streams > GCN10_N_RASTERS || W <= 0 || rows < 0)
        return fail(GCN10_E_INVAL, "%s: bad shape %d rasters of %d x %d", who, streams, W, rows);
    if (rows == 0)
        return GCN10_OK;
    if (!arena || !table || !cursor)
        return fail(GCN10_E_INVAL, "%s: null pointer", who);
    if ((reinterpret_cast<uintptr_t>(arena) & 15u) != 0)
        return fail(GCN10_E_INVAL, "%s: arena must be 16-byte aligned", who);
    // stream offsets are 32-bit table entries with 0xfffffffe / 0xffffffff reserved
    if (arena_cap >= 0xfffffffeull)
        return fail(GCN10_E_INVAL, "%s: an arena of %zu bytes does not fit 32-bit stream offsets "
                                   "(use fewer rows per strip)", who, arena_cap);
    job->arena = arena;
    job->arena_cap = arena_cap;
    job->table = table;
    job->sizes = table;
    job->cursor = cursor;
    job->W = (uint32_t)W;
    job->rows = (uint32_t)rows;
    job->across = ((uint32_t)W + kTile - 1) / kTile;
    job->down = ((uint32_t)rows + kTile - 1) / kTile;
    const uint64_t n_tiles = (uint64_t)job->across * job->down * (uint64_t)streams;
    if (n_tiles > 0x7fffffffull)
        return fail(GCN10_E_INVAL, "%s: too many tiles", who);
    job->n_tiles = (uint32_t)n_tiles;
    return GCN10_OK;
}

size_t arena_bound(int W, int rows, int n_rasters, size_t max_stream)
{
    if (W <= 0 || rows <= 0 || n_rasters <= 0)
        return 0;
    const size_t across = ((size_t)W + kTile - 1) / kTile, down = ((size_t)rows + kTile - 1) / kTile;
    const size_t slot = (max_stream + kSlotAlign - 1) / kSlotAlign * kSlotAlign;
    // + the pads that bring every raster's extent to a multiple of the largest segment alignment
    return across * down * (size_t)n_rasters * slot + (size_t)n_rasters * 4096u;
}

int launch_arena_place(gcn10_gpu_ctx *ctx, const TileJob &job, hipStream_t s)
{
    hipLaunchKernelGGL(deflate_place_kernel, dim3(1), dim3(kPlaceThreads), 0, s, job, job.across * job.down,
                       (uint32_t)ctx->opt.arena_segment_align);
    HIP_TRY(hipGetLastError());
    return GCN10_OK;
}

}  // namespace gcn10
