/* levels.c -- the overview levels of a staged block on the device (DESIGN.md "Cloud Optimized GeoTIFF").
 *
 * The writer (pipeline.c, encode_overviews) encodes them into the files and the verifier (verify.c) compares the files'
 * levels with them: both get them from here, so what is verified is what would be written.
 */
#include "pipeline_internal.h"

#include <stdlib.h>

#define wlog gcn10_wlog

int gcn10_level_nearest(struct worker *w, const struct block_in *in, int k, int *Wk_out, int *Hk_out,
                        const int32_t **d_cj)
{
    const struct gcn10_gpu_api *g = w->run->gpu;
    const int W = in->W, H = in->H;
    /* the buffers are sized for level 1, the largest: the levels of a block share them, so only the first call of a
     * block can grow them (the host copy of the maps, a few KB, is made per level).  A level's ci, padded to a
     * multiple of 4 entries, then its cj: at most W1 + 3 + H1 entries */
    const size_t W1 = (size_t)gcn10_level_dim(W, 1), H1 = (size_t)gcn10_level_dim(H, 1), n_idx = W1 + 4 + H1;
    const int Wk = gcn10_level_dim(W, k), Hk = gcn10_level_dim(H, k), half = 1 << (k - 1);
    /* cj of the level right after its ci, 16-byte aligned */
    const size_t cj_at = ((size_t)Wk + 3) & ~(size_t)3;
    int32_t *idx;
    int rc = -1;

    if (gcn10_ensure_dev_on(w, w->ctx, (void **)&w->d_ov, &w->ov_cap, W1 * H1 + 16) != 0 ||
        gcn10_ensure_dev_on(w, w->ctx, (void **)&w->d_ov_idx, &w->ov_idx_cap, n_idx * sizeof *idx) != 0)
        return -1;
    idx = malloc(n_idx * sizeof *idx);
    if (!idx) {
        wlog(w, "ERROR", true, "malloc failed for overview index maps");
        return -1;
    }
    /* the level's pixel x samples the block's pixel x * 2^k + 2^(k-1) (the last one at the edge): its landcover is
     * gathered so, and its soil index maps are the block's composed with the same sampling */
    for (int x = 0; x < Wk; x++)
        idx[x] = in->h_ci[(int64_t)x * (1 << k) + half < W ? (int64_t)x * (1 << k) + half : W - 1];
    for (int y = 0; y < Hk; y++)
        idx[cj_at + y] = in->h_cj[(int64_t)y * (1 << k) + half < H ? (int64_t)y * (1 << k) + half : H - 1];
    if (g->overview_nearest(w->ctx, in->d_block, W, H, k, w->d_ov, w->s_kernel) != 0 ||
        g->memcpy_h2d(w->ctx, w->d_ov_idx, idx, (cj_at + (size_t)Hk) * sizeof *idx, w->s_kernel) != 0 ||
        g->stream_sync(w->ctx, w->s_kernel) != 0 ||
        g->prepare_tile(w->ctx, in->d_coarse, in->hsx, in->hsy, w->d_ov_idx, Wk, w->s_kernel) != 0)
        wlog(w, "ERROR", true, "gpu: %s", g->last_error());
    else
        rc = 0;
    free(idx);
    *Wk_out = Wk;
    *Hk_out = Hk;
    *d_cj = w->d_ov_idx + cj_at;
    return rc;
}

int gcn10_levels_average(struct worker *w, const struct block_in *in, int L, int strip_rows,
                         uint8_t *levels[GCN10_N_RASTERS * GCN10_COG_MAX_LEVELS])
{
    struct run *r = w->run;
    const struct gcn10_gpu_api *g = r->gpu;
    const int W = in->W, H = in->H;
    size_t lvl_off[GCN10_COG_MAX_LEVELS + 1], total = 0;

    /* raster by raster, each raster's levels 1 .. L one after the other, 256-byte aligned */
    for (int k = 1; k <= L; k++) {
        lvl_off[k] = total;
        total += ((size_t)gcn10_level_dim(W, k) * (size_t)gcn10_level_dim(H, k) + 255) & ~(size_t)255;
    }
    if (gcn10_ensure_dev_on(w, w->ctx, (void **)&w->d_ov, &w->ov_cap, total * (size_t)r->n_sel + 16) != 0)
        return -1;
    for (int q = 0; q < r->n_sel; q++)
        for (int k = 1; k <= L; k++)
            levels[q * L + k - 1] = w->d_ov + (size_t)q * total + lvl_off[k];
    for (int y0 = 0; y0 < H; y0 += strip_rows) {
        const int rows = H - y0 < strip_rows ? H - y0 : strip_rows;

        GPU_OR_RETURN(w, -1, g->overview_average(w->ctx, in->d_block, W, H, y0, rows, in->d_cj, r->cond_mask,
                                                 r->table_mask, L, levels, w->s_kernel));
    }
    return 0;
}
