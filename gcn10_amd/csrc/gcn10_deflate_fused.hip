// gcn10_deflate_fused.hip -- the fused tile encoder: 18 zlib streams per 256x256 tile position
// straight from the landcover strip and the prepared soil codes; no CN raster in HBM.
// What it replaces and the stream format: see gcn10_deflate.hip.
//
// The 18 rasters of a block are functions of the same (landcover,
// soil) pixel pairs, so their repeats line up.  Pixels are reduced to a CLASS id (two
// pixels share a class iff all 18 rasters agree on them; gcn10_gpu_set_tables builds
// the map), the class tile is loaded, masked and tokenised ONCE per tile position, and
// the 18 streams are produced from it: no CN raster is ever written to or read from HBM
// (24.6 GB written + 2 x 23.3 GB read per block in the unfused path -> 1.4 GB read).
// A match of the class stream is a match in every raster; a raster's own extra repeats
// (two classes with the same value in that raster) are coded as literals, which costs a
// little compression.  Three launches per strip:
//   F-A  gcn10_deflate_fused_stats.hpp.  One workgroup per tile position: class tile, match
//        masks, greedy parse of every row, the position's 16-bit token stream -> workspace;
//        per raster the literal statistics (class counts mapped through class_val) and the
//        Adler-32 (per-class pixel counts and position-weight sums); drained/undrained aliases
//   B    gcn10_deflate_codes.hip.  Code construction per (raster, tile), the per-raster
//        encoder's pass unchanged
//   F-C  gcn10_deflate_fused_emit.hpp.  One workgroup per (position, group of kGroup rasters),
//        token-parallel: prefix sums of the tokens' code lengths place their bits, words go
//        straight to the arena.  Its default form places the streams itself; the lock-step form
//        (option fused_emit = 0) runs behind pass B' (gcn10_arena_place.hip), a fourth launch
// The two passes are headers of this one translation unit: gcn10_deflate_fused_internal.hpp says why.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "gcn10_deflate_fused_emit.hpp"
#include "gcn10_deflate_fused_internal.hpp"
#include "gcn10_deflate_fused_stats.hpp"
#include "gcn10_deflate_internal.hpp"
#include "gcn10_gpu.h"
#include "gcn10_gpu_internal.hpp"

using gcn10::as_stream;
using gcn10::fail;
using gcn10::use_device;

extern "C" {

int gcn10_gpu_deflate_fused_available(gcn10_gpu_ctx *ctx)
{
    return ctx && ctx->n_tables > 0 && ctx->n_classes > 0 ? 1 : 0;
}

int gcn10_gpu_deflate_fused_strip(gcn10_gpu_ctx *ctx, const uint8_t *esa, int W, int rows, const int32_t *cj,
                                  unsigned cond_mask, unsigned table_mask, uint8_t *arena_dev, size_t arena_cap,
                                  uint32_t *table_dev, unsigned long long *cursor_dev, gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    const char *const who = "gcn10_gpu_deflate_fused_strip";
    hipStream_t s = as_stream(ctx, stream);
    if ((rc = gcn10::check_tables(ctx, who)) != GCN10_OK)
        return rc;
    if (ctx->n_classes == 0)
        return fail(GCN10_E_STATE, "gcn10_gpu_deflate_fused_strip: the lookup tables define more than 256 pixel "
                                   "classes; use gcn10_gpu_cn_strip + gcn10_gpu_deflate_strip");
    FusedJob job;
    memset(&job, 0, sizeof job);
    if ((rc = gcn10::bind_soil(ctx, who, W, s, cj, &job.soil)) != GCN10_OK)
        return rc;
    if (rows < 0)
        return fail(GCN10_E_INVAL, "gcn10_gpu_deflate_fused_strip: rows=%d", rows);
    if ((rc = gcn10::check_masks(ctx, who, cond_mask, table_mask)) != GCN10_OK)
        return rc;
    for (int r = 0; r < GCN10_N_RASTERS; r++)
        if (gcn10::selected(r, cond_mask, table_mask))
            job.sel[job.n_sel++] = (uint8_t)r;
    rc = gcn10::tile_job_setup(who, W, rows, (int)job.n_sel, arena_dev, arena_cap, table_dev, cursor_dev, &job.t);
    if (rc || job.t.n_tiles == 0)
        return rc;                  // refused, or an empty strip
    if (!esa || !cj)
        return fail(GCN10_E_INVAL, "%s: null pointer", who);
    job.esa = esa;
    job.class_of = ctx->d_class_of;
    job.seg_align = (uint32_t)ctx->opt.arena_segment_align;
    const uint32_t positions = job.t.across * job.t.down, nblocks = job.t.n_tiles;
    // (pass F-C adds a raster's stream sizes up in 32 bits; with the 4 GB arena limit of the job setup only a strip
    // far beyond any arena can get here)
    if ((uint64_t)positions * (uint64_t)(kMaxStream + kSlotAlign) >= 0xffffffffull)
        return fail(GCN10_E_INVAL, "tile encoder: %u tile positions in one strip (use fewer rows per strip)", positions);

    // workspace: statistics + code books per (raster, tile), token tiles + match starts per position
    const size_t stats_bytes = ((size_t)nblocks * ((size_t)kHistWords * 4 + (size_t)kBookBytes) + 255) & ~(size_t)255;
    const size_t tok_bytes = (size_t)positions * kTokStride * sizeof(uint16_t);
    const size_t ntok_bytes = ((size_t)positions * sizeof(uint32_t) + 15) & ~(size_t)15;
    const size_t need = stats_bytes + tok_bytes + ntok_bytes + (size_t)nblocks * 8 + (size_t)job.n_sel * ((positions + 63u) / 64u) * 4;
    rc = gcn10::grow_workspace(&ctx->ws.deflate, &ctx->ws.deflate_cap, need);
    if (rc)
        return rc;
    job.t.hist = reinterpret_cast<uint32_t *>(ctx->ws.deflate);
    job.t.books = reinterpret_cast<uint8_t *>(ctx->ws.deflate) + (size_t)nblocks * kHistWords * 4;
    job.tok = reinterpret_cast<uint16_t *>(reinterpret_cast<uint8_t *>(ctx->ws.deflate) + stats_bytes);
    job.n_tok = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(ctx->ws.deflate) + stats_bytes + tok_bytes);
    // the wave-independent pass F-C places the streams itself, every workgroup from all the sizes: those must not be
    // the table the workgroups write the offsets to
    if (ctx->opt.fused_emit != 0) {
        job.t.sizes = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(ctx->ws.deflate) + stats_bytes + tok_bytes + ntok_bytes);
        job.t.chunk_tot = job.t.sizes + (size_t)nblocks * 2;        // zeroed by pass F-A, added to by pass B
        job.t.n_chunks = (positions + 63u) / 64u;
    }

    if ((rc = launch_fused_stats(ctx, job, s)) != GCN10_OK)
        return rc;
    // (pass B' as a launch of its own only for the lock-step form of pass F-C: the wave-independent form places its streams itself)
    if ((rc = gcn10::deflate_launch_codes(ctx, job.t, nblocks, s, ctx->opt.fused_emit == 0)) != GCN10_OK)
        return rc;
    return launch_fused_emit(ctx, job, s);
}

}  // extern "C"
