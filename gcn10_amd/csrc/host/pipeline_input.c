/* pipeline_input.c -- the input side of a block worker: one block ahead of the encoder.
 *
 * What it replaces: the front half of process_block() (/root/reference/src/cn.c:155-232): the
 * block's bbox, load_raster() of the landcover window (src/raster.c:106-189, one blocking
 * GDALRasterIO into a malloc'ed buffer) and of the soil window, and the index arithmetic of the
 * resample.  In the reference that is serial with everything else a rank does.  Here every block
 * worker has an input thread with a GPU context and stream of its own: while the worker encodes
 * block N, the thread
 *   - takes the next block id from the run's counter and computes its windows (geo.c, bit exact),
 *   - reads the soil window and builds the index maps into pinned memory, copies them to HBM,
 *   - PLANS the landcover window (raster.c / tiff_window.c: which chunks of which files, clipped how),
 *     has the I/O pool pread the chunks -- compressed or raw, as they lie in the files -- into
 *     a ring of pinned buffers, and copies batch k to HBM (hipMemcpyAsync on its stream) while the
 *     pool fills batch k+1: the "pinned-host staging, double-buffered" of the north star,
 *   - launches gcn10_gpu_inflate_tiles on them: DEFLATE and LZW tiles are decoded, raw tiles untiled, TIFF
 *     predictor 2 undone, all in HBM, into the row-major window d_block (LZW with gpu_inflate_lzw=1, the
 *     default, when the GPU library reports the codec),
 *   - (windows the GPU side cannot take -- PackBits, overlapping mosaic sources, LZW with gpu_inflate_lzw=0
 *     -- are read by the host reader strip by strip into the same ring and copied up the same way),
 *   - records one event behind all of it and hands the slot to the worker.
 * Two slots per worker: the block being encoded and the one being staged, so at most two blocks'
 * input are resident per worker.  prefetch_blocks=0 runs the same code on the worker thread itself.
 */
#include "pipeline_internal.h"

#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#define now_seconds gcn10_now_seconds
#define wlog gcn10_wlog

/* longest stream first among the compressed ones (one workgroup decodes one stream and the GPU hands
 * workgroups out in index order: the stragglers start first); raw chunks keep their file order behind them */
static int by_size_desc(const void *a, const void *b)
{
    const struct gcn10_chunk_ref *x = a, *y = b;
    const int xr = (x->flags & GCN10_TILE_RAW) != 0, yr = (y->flags & GCN10_TILE_RAW) != 0;

    if (xr != yr)
        return xr - yr;
    if (xr)
        return x->file_off < y->file_off ? -1 : (x->file_off > y->file_off ? 1 : 0);
    return x->nbytes < y->nbytes ? 1 : (x->nbytes > y->nbytes ? -1 : 0);
}

/* The landcover window through the GPU side.  0 = issued on s_in; 1 = this window needs the host reader;
 * -1 = the window cannot be read (logged; the block is skipped as after a failed load_raster,
 * src/cn.c:188-192); -2 = device error (logged; fatal for the run). */
static int stage_planned(struct worker *w, struct block_in *in)
{
    struct run *r = w->run;
    const struct gcn10_gpu_api *g = r->gpu;
    struct gcn10_job_list *jl = &in->jl;
    struct gcn10_read_plan plan;
    char err[1024] = "";
    int rc;
    size_t comp_bytes = 0, largest = RING_BYTES, n_bad = 0;
    const int W = in->W, H = in->H;
    double t0 = now_seconds();

    rc = gcn10_raster_plan_window_codecs(w->esa, in->xoff, in->yoff, W, H, r->inflate_codecs, &plan, err, sizeof err);
    if (rc > 0)
        return 1;
    if (rc < 0) {
        wlog(w, "ERROR", true, "%s", err);
        wlog(w, "ERROR", true, "esa load failed for block %d", in->block_id);
        return -1;
    }
    if (!getenv("GCN10_INFLATE_FILE_ORDER"))      /* (A/B switch for tools/) */
        qsort(plan.chunks, plan.n, sizeof *plan.chunks, by_size_desc);
    rc = -2;
    if (gcn10_job_list_ensure(g, w->in_ctx, jl, plan.n, 0) != 0)
        goto gpu_fail;
    for (size_t i = 0; i < plan.n; i++) {
        const struct gcn10_chunk_ref *c = &plan.chunks[i];
        const size_t slot = gcn10_chunk_slot(c->nbytes);

        gcn10_inflate_job_from_chunk(&jl->h_jobs[i], c, comp_bytes, (uint64_t)c->dst_y * (uint64_t)W + c->dst_x);
        comp_bytes += slot;
        if (slot > largest)
            largest = slot;
        jl->h_status[i] = 0xffffffffu;
    }
    if (gcn10_ensure_dev_on(w, w->in_ctx, (void **)&in->d_comp, &in->d_comp_cap, comp_bytes + 16) != 0)
        goto out;               /* logged */
    /* the ring takes the largest chunk: none is too large to stage */
    if (gcn10_stager_ensure(&w->ring, largest) != 0 ||
        (plan.covered < (uint64_t)W * (uint64_t)H &&
         g->memset(w->in_ctx, in->d_block, 0, (size_t)W * (size_t)H, w->s_in) != 0) ||
        gcn10_stager_stage(&w->ring, plan.chunks, jl->h_jobs, plan.n, in->d_comp, w->s_in, jl->bad) != 0)
        goto gpu_fail;
    w->t_read += now_seconds() - t0;
    for (size_t i = 0; i < plan.n; i++)
        n_bad += jl->bad[i] != 0;
    if (n_bad) {
        wlog(w, "ERROR", true, "gdalrasterio error: cannot read the landcover tiles of the window %d,%d %dx%d",
             in->xoff, in->yoff, W, H);
        wlog(w, "ERROR", true, "esa load failed for block %d", in->block_id);
        rc = -1;
        goto out;
    }
    if (plan.n > 0 &&
        (g->memcpy_h2d(w->in_ctx, jl->d_jobs, jl->h_jobs, plan.n * sizeof *jl->h_jobs, w->s_in) != 0 ||
         g->memcpy_h2d(w->in_ctx, jl->d_status, jl->h_status, plan.n * 4, w->s_in) != 0 ||
         g->inflate_tiles(w->in_ctx, in->d_comp, jl->d_jobs, (int)plan.n, plan.max_chunk_bytes ? plan.max_chunk_bytes : 16,
                          in->d_block, (size_t)W, jl->d_status, w->s_in) != 0 ||
         g->memcpy_d2h(w->in_ctx, jl->h_status, jl->d_status, plan.n * 4, w->s_in) != 0))
        goto gpu_fail;
    in->n_inflate = plan.n;
    w->n_win_gpu++;
    for (size_t i = 0; i < plan.n; i++)
        if (plan.chunks[i].flags & GCN10_TILE_LZW) {
            w->n_win_gpu_lzw++;
            break;
        }
    rc = 0;
    goto out;

gpu_fail:
    /* a device error (allocation, copy, launch) is not a failed load_raster: it ends the run like every
     * other GPU error of process_block, instead of skipping the block */
    wlog(w, "ERROR", true, "gpu: %s", g->last_error());
    rc = -2;
out:
    /* the files may close: the bytes are in pinned memory or further */
    gcn10_read_plan_free(&plan);
    return rc;
}

/* The landcover window through the host reader, a band of rows at a time: decoded by the I/O pool straight
 * into a pinned staging buffer (replaces the malloc + GDALRasterIO of src/raster.c:169-178), copied up
 * while the next band is decoded.  0, -1 (logged, block skipped) or -2 (device error). */
static int stage_host(struct worker *w, struct block_in *in)
{
    struct run *r = w->run;
    const struct gcn10_gpu_api *g = r->gpu;
    const int W = in->W, H = in->H;
    char err[1024] = "";
    int band, k = 0;

    GPU_OR_RETURN(w, -2, gcn10_stager_ensure(&w->ring, (size_t)W * 256 > (size_t)RING_BYTES ? (size_t)W * 256
                                                                                              : (size_t)RING_BYTES));
    band = (int)(w->ring.cap / (size_t)W);
    if (band > r->strip_rows)
        band = r->strip_rows;           /* the granularity of round 1-2's per-strip reads */
    for (int y0 = 0; y0 < H; y0 += band) {
        const int rows = H - y0 < band ? H - y0 : band;
        double t0 = now_seconds();
        int rc;

        GPU_OR_RETURN(w, -2, gcn10_stager_take(&w->ring, k));
        rc = gcn10_raster_read_mt(w->esa, in->xoff, in->yoff + y0, W, rows, w->ring.h[k], r->pool, err, sizeof err);
        w->t_read += now_seconds() - t0;
        if (rc != 0) {
            wlog(w, "ERROR", true, "%s", err);
            wlog(w, "ERROR", true, "esa load failed for block %d", in->block_id);
            return -1;
        }
        GPU_OR_RETURN(w, -2, g->memcpy_h2d(w->in_ctx, in->d_block + (size_t)y0 * (size_t)W, w->ring.h[k],
                                           (size_t)W * (size_t)rows, w->s_in));
        GPU_OR_RETURN(w, -2, gcn10_stager_sent(&w->ring, k, w->s_in));
        k = (k + 1) % N_RING;
    }
    return 0;
}

/* One block from its id to "everything it needs is on its way to HBM": the front half of process_block
 * (src/cn.c:155-232).  Returns the slot's outcome: 0, 1 (skipped, logged) or -1 (fatal). */
static int fill_block(struct worker *w, struct block_in *in, int block_id)
{
    struct run *r = w->run;
    const struct gcn10_gpu_api *g = r->gpu;
    char err[1024] = "";
    double esa_t[6], soil_t[6], soil_gt[6];
    int esa_rx, esa_ry, soil_rx, soil_ry, sxoff, syoff, bi, rc;
    double t_mark;

    in->block_id = block_id;
    in->n_inflate = 0;
    if (!w->esa) {
        wlog(w, "ERROR", true, "esa load failed for block %d", block_id);          /* src/cn.c:189 */
        return 1;
    }
    if (!w->soil) {
        wlog(w, "ERROR", true, "hysogs load failed for block %d", block_id);
        return 1;
    }
    /* block geometry: attribute filter "ID"=<id>, first feature (src/cn.c:162-184) */
    bi = gcn10_blocks_find(&r->blocks, block_id);
    if (bi < 0) {
        wlog(w, "ERROR", true, "block %d not found", block_id);                     /* src/cn.c:173 */
        return 1;
    }
    /* landcover window (src/cn.c:187-192, src/raster.c:126-162) */
    gcn10_raster_info(w->esa, &esa_rx, &esa_ry, esa_t);
    if (gcn10_raster_window(esa_t, esa_rx, esa_ry, r->blocks.bbox[bi], &in->xoff, &in->yoff, &in->W, &in->H,
                            in->gt) != 0) {
        wlog(w, "ERROR", true, "invalid raster bounds for %s", r->cfg.esa_data_path);   /* src/raster.c:143 */
        wlog(w, "ERROR", true, "esa load failed for block %d", block_id);               /* src/cn.c:189 */
        return 1;
    }
    /* soil window (src/cn.c:195-203) */
    gcn10_raster_info(w->soil, &soil_rx, &soil_ry, soil_t);
    if (gcn10_raster_window(soil_t, soil_rx, soil_ry, r->blocks.bbox[bi], &sxoff, &syoff, &in->hsx, &in->hsy,
                            soil_gt) != 0) {
        wlog(w, "ERROR", true, "invalid raster bounds for %s", r->cfg.hysogs_data_path);
        wlog(w, "ERROR", true, "hysogs load failed for block %d", block_id);            /* src/cn.c:198 */
        return 1;
    }
    if ((long long)in->W * (long long)in->H > INT_MAX) {
        /* the reference's int npix (src/cn.c:208) overflows here; refuse instead */
        wlog(w, "ERROR", true, "block %d: %d x %d pixels exceed 2^31-1", block_id, in->W, in->H);
        return 1;
    }
    /* soil window and index maps in pinned memory owned by the slot: their copies to the GPU need no wait */
    if (gcn10_ensure_pinned_on(w, w->in_ctx, (void **)&in->h_coarse, &in->h_coarse_cap, (size_t)in->hsx * (size_t)in->hsy) != 0 ||
        gcn10_ensure_pinned_on(w, w->in_ctx, (void **)&in->h_ci, &in->h_ci_cap, (size_t)in->W * sizeof *in->h_ci) != 0 ||
        gcn10_ensure_pinned_on(w, w->in_ctx, (void **)&in->h_cj, &in->h_cj_cap, (size_t)in->H * sizeof *in->h_cj) != 0) {
        wlog(w, "ERROR", true, "malloc failed for hysogs resampling, block %d", block_id); /* src/cn.c:211 */
        return -1;
    }
    t_mark = now_seconds();
    /* the soil raster is a global file of full-width strips: a block's window touches ~1440 of
     * them, decoded concurrently on the I/O pool and only as far as the window reaches */
    if (gcn10_raster_read_mt(w->soil, sxoff, syoff, in->hsx, in->hsy, in->h_coarse, r->pool, err, sizeof err) != 0) {
        wlog(w, "ERROR", true, "%s", err);
        wlog(w, "ERROR", true, "hysogs load failed for block %d", block_id);
        return 1;
    }
    gcn10_build_index_maps(in->gt, soil_gt, in->W, in->H, in->hsx, in->hsy, in->h_ci, in->h_cj);   /* src/cn.c:218-229 */
    w->t_soil += now_seconds() - t_mark;

    if (gcn10_ensure_dev_on(w, w->in_ctx, (void **)&in->d_coarse, &in->coarse_cap, (size_t)in->hsx * (size_t)in->hsy) != 0 ||
        gcn10_ensure_dev_on(w, w->in_ctx, (void **)&in->d_ci, &in->ci_cap, (size_t)in->W * 4) != 0 ||
        gcn10_ensure_dev_on(w, w->in_ctx, (void **)&in->d_cj, &in->cj_cap, (size_t)in->H * 4) != 0 ||
        gcn10_ensure_dev_on(w, w->in_ctx, (void **)&in->d_block, &in->block_cap, (size_t)in->W * (size_t)in->H) != 0)
        return -1;
    if (g->memcpy_h2d(w->in_ctx, in->d_coarse, in->h_coarse, (size_t)in->hsx * (size_t)in->hsy, w->s_in) != 0 ||
        g->memcpy_h2d(w->in_ctx, in->d_ci, in->h_ci, (size_t)in->W * 4, w->s_in) != 0 ||
        g->memcpy_h2d(w->in_ctx, in->d_cj, in->h_cj, (size_t)in->H * 4, w->s_in) != 0) {
        wlog(w, "ERROR", true, "gpu: %s", g->last_error());
        return -1;
    }
    /* the landcover window: chunks as they lie in the files -> HBM -> decoded / untiled there; what the GPU
     * side cannot take, and everything with gpu_inflate=0, through the host reader */
    rc = r->gpu_inflate ? stage_planned(w, in) : 1;
    if (rc == 1) {
        w->n_win_host++;
        rc = stage_host(w, in);
    }
    if (rc == 0 && g->event_record(w->in_ctx, in->ev_ready, w->s_in) != 0) {
        wlog(w, "ERROR", true, "gpu: %s", g->last_error());
        rc = -2;
    }
    if (rc != 0) {
        /* nothing of a block that is not going to be encoded may still be in flight when its slot is reused */
        g->stream_sync(w->in_ctx, w->s_in);
        gcn10_stager_idle(&w->ring);
        return rc == -2 ? -1 : 1;
    }
    /* no file yet, and rasters of the window's size unless the mode's plan says otherwise */
    memset(in->tifs, 0, sizeof in->tifs);
    in->tifs_ok = false;
    in->out_W = in->W;
    in->out_H = in->H;
    memcpy(in->out_gt, in->gt, sizeof in->out_gt);
    /* what the mode makes of the block on the host (the zones or the grid's cells over it, its grid of aggregated
     * cells), here on the input side: it overlaps the block before */
    if (r->mode->plan_block && (rc = r->mode->plan_block(w, in, r->blocks.bbox[bi])) != 0) {
        g->stream_sync(w->in_ctx, w->s_in);
        gcn10_stager_idle(&w->ring);
        return rc;
    }
    if (!r->mode->writes_block_files)
        return 0;
    /* the block's 18 files, while the copies and the decoder run (the reference creates each raster's file
     * inside save_raster, after computing it: src/raster.c:204; an existing raster of that name is untouched
     * until this one is complete either way: files are written as <name>.part) */
    return gcn10_create_outputs(w, in) < 0 ? -1 : 0;    /* (1: logged; the worker finds tifs_ok false and gives it up) */
}

/* takes the next block of the queue and fills slot `in` with it; false at the end of the queue */
static bool take_and_fill(struct worker *w, struct block_in *in)
{
    struct run *r = w->run;
    int i = atomic_fetch_add(&r->next_block, 1);
    double t0;

    if (i >= r->n_blocks || atomic_load(&r->fatal))
        return false;
    wlog(w, "INFO", true, "processing block %d", r->block_ids[i]);          /* src/main.c:172-173 */
    t0 = now_seconds();
    if (w->t_first_block == 0.0)
        w->t_first_block = t0;
    in->outcome = fill_block(w, in, r->block_ids[i]);
    w->t_in_busy += now_seconds() - t0;
    if (in->outcome < 0)
        atomic_store(&r->fatal, 1);     /* where the reference calls MPI_Abort */
    return true;
}

static void *input_main(void *arg)
{
    struct worker *w = arg;

    for (int n = 0;; n++) {
        struct block_in *in = &w->in[n % N_IN];
        bool more;

        pthread_mutex_lock(&w->in_mu);
        while (in->state != IN_FREE && !w->in_stop)
            pthread_cond_wait(&w->in_cv, &w->in_mu);
        if (w->in_stop) {
            pthread_mutex_unlock(&w->in_mu);
            { w->in_cpu_seconds = gcn10_thread_cpu_seconds(); return NULL; }
        }
        in->state = IN_FILLING;
        pthread_mutex_unlock(&w->in_mu);

        more = take_and_fill(w, in);

        pthread_mutex_lock(&w->in_mu);
        in->state = more ? IN_READY : IN_END;
        pthread_cond_broadcast(&w->in_cv);
        pthread_mutex_unlock(&w->in_mu);
        if (!more)
            { w->in_cpu_seconds = gcn10_thread_cpu_seconds(); return NULL; }
    }
}

int gcn10_input_setup(struct worker *w)
{
    const struct gcn10_gpu_api *g = w->run->gpu;

    pthread_mutex_init(&w->in_mu, NULL);
    pthread_cond_init(&w->in_cv, NULL);
    /* a context of its own: the input side calls the GPU library concurrently with the worker, and a
     * context is not shared between threads (include/gcn10_gpu.h); device memory and events are valid
     * in both, they belong to the device */
    GPU_OR_RETURN(w, -2, g->init(w->device, &w->in_ctx));
    if (w->run->event_sleep_us > 0 && g->set_option)
        (void)g->set_option(w->in_ctx, "event_sync_sleep_us", w->run->event_sleep_us);
    GPU_OR_RETURN(w, -2, g->stream_create(w->in_ctx, &w->s_in));
    /* (its buffers come with the first block) */
    GPU_OR_RETURN(w, -2, gcn10_stager_setup(&w->ring, g, w->in_ctx, w->run->pool, &w->run->pinned_bytes, N_RING,
                                            0));
    for (int k = 0; k < N_IN; k++)
        GPU_OR_RETURN(w, -2, g->event_create(w->in_ctx, &w->in[k].ev_ready));
    return 0;
}

int gcn10_input_start(struct worker *w)
{
    if (!w->run->prefetch)
        return 0;
    if (pthread_create(&w->in_thread, NULL, input_main, w) != 0) {
        wlog(w, "ERROR", true, "cannot start the input thread");
        return -1;
    }
    w->in_thread_started = true;
    return 0;
}

struct block_in *gcn10_input_next(struct worker *w)
{
    struct block_in *in;

    if (!w->in_thread_started) {
        /* no input thread: the worker stages its own block, in turn with encoding it */
        in = &w->in[0];
        if (!take_and_fill(w, in))
            return NULL;
        in->state = IN_READY;
        return in;
    }
    in = &w->in[w->in_seq % N_IN];
    {
        double t0 = now_seconds();

        pthread_mutex_lock(&w->in_mu);
        while (in->state != IN_READY && in->state != IN_END)
            pthread_cond_wait(&w->in_cv, &w->in_mu);
        pthread_mutex_unlock(&w->in_mu);
        w->t_in_wait += now_seconds() - t0;
    }
    return in->state == IN_READY ? in : NULL;
}

void gcn10_input_release(struct worker *w, struct block_in *in)
{
    pthread_mutex_lock(&w->in_mu);
    in->state = IN_FREE;
    pthread_cond_broadcast(&w->in_cv);
    pthread_mutex_unlock(&w->in_mu);
}

void gcn10_input_stop(struct worker *w)
{
    if (!w->in_thread_started)
        return;
    pthread_mutex_lock(&w->in_mu);
    w->in_stop = true;
    pthread_cond_broadcast(&w->in_cv);
    pthread_mutex_unlock(&w->in_mu);
    pthread_join(w->in_thread, NULL);
    w->in_thread_started = false;
}

void gcn10_input_teardown(struct worker *w)
{
    const struct gcn10_gpu_api *g = w->run->gpu;

    gcn10_input_stop(w);
    if (w->in_ctx) {
        g->device_sync(w->in_ctx);
        for (int k = 0; k < N_IN; k++) {
            struct block_in *in = &w->in[k];

            gcn10_abort_outputs(in);        /* a staged block the worker never took */
            if (w->run->mode->plan_free)
                w->run->mode->plan_free(in);
            if (in->h_coarse) g->host_free(w->in_ctx, in->h_coarse);
            if (in->h_ci) g->host_free(w->in_ctx, in->h_ci);
            if (in->h_cj) g->host_free(w->in_ctx, in->h_cj);
            if (in->d_coarse) g->free(w->in_ctx, in->d_coarse);
            if (in->d_ci) g->free(w->in_ctx, in->d_ci);
            if (in->d_cj) g->free(w->in_ctx, in->d_cj);
            if (in->d_block) g->free(w->in_ctx, in->d_block);
            if (in->d_comp) g->free(w->in_ctx, in->d_comp);
            gcn10_job_list_free(g, w->in_ctx, &in->jl);
            if (in->ev_ready) g->event_destroy(w->in_ctx, in->ev_ready);
            memset(in, 0, sizeof *in);
        }
        gcn10_stager_teardown(&w->ring);
        if (w->s_in) g->stream_destroy(w->in_ctx, w->s_in);
        g->destroy(w->in_ctx);
        w->in_ctx = NULL;
    }
    pthread_mutex_destroy(&w->in_mu);
    pthread_cond_destroy(&w->in_cv);
}
