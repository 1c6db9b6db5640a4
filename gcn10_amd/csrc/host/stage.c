/* stage.c -- chunks of TIFF files, as they lie there, on their way to gcn10_gpu_inflate_tiles.
 *
 * The input side of a block worker (pipeline_input.c: the landcover window) and the verifier (verify.c: a strip of the
 * 18 written rasters) both hold a read plan -- which bytes of which files -- and want those bytes in device memory, each
 * chunk at its in_off with 16 zero bytes behind it.  Here is the one way there: the I/O pool preads batch b of the
 * chunks into pinned buffer b % n while the copy of batch b - 1 to the device is in flight.  The file knows nothing of
 * workers or logs: it works on a context, a stream and a pool, and hands device errors back to its caller.
 */
#include "pipeline_internal.h"

#include <string.h>
#include <unistd.h>

enum { SLICE = 32 };                /* chunks per pool job */

size_t gcn10_chunk_slot(uint32_t nbytes)
{
    return (((size_t)nbytes + 15) & ~(size_t)15) + 16;
}

void gcn10_inflate_job_from_chunk(gcn10_inflate_tile *j, const struct gcn10_chunk_ref *c, uint64_t in_off,
                                  uint64_t dst_off)
{
    j->in_off = in_off;
    j->in_len = c->nbytes;
    j->out_len = c->out_len;
    j->chunk_w = c->chunk_w;
    j->src_x = c->src_x;
    j->src_y = c->src_y;
    j->copy_w = c->copy_w;
    j->copy_h = c->copy_h;
    j->flags = c->flags;
    j->dst_off = dst_off;
}

void gcn10_job_list_free(const struct gcn10_gpu_api *g, gcn10_gpu_ctx *ctx, struct gcn10_job_list *l)
{
    if (l->h_jobs) g->host_free(ctx, l->h_jobs);
    if (l->d_jobs) g->free(ctx, l->d_jobs);
    if (l->h_status) g->host_free(ctx, l->h_status);
    if (l->d_status) g->free(ctx, l->d_status);
    if (l->bad) g->host_free(ctx, l->bad);
    memset(l, 0, sizeof *l);
}

int gcn10_job_list_ensure(const struct gcn10_gpu_api *g, gcn10_gpu_ctx *ctx, struct gcn10_job_list *l, size_t n,
                          size_t keep)
{
    gcn10_inflate_tile *h_jobs = NULL;
    uint32_t *h_status = NULL;
    int rc;

    if (n <= l->cap)
        return 0;
    if ((rc = g->host_alloc(ctx, n * sizeof *h_jobs, (void **)&h_jobs)) != 0)
        return rc;
    if ((rc = g->host_alloc(ctx, n * sizeof *h_status, (void **)&h_status)) != 0) {
        g->host_free(ctx, h_jobs);
        return rc;
    }
    if (keep > 0) {
        memcpy(h_jobs, l->h_jobs, keep * sizeof *h_jobs);
        memcpy(h_status, l->h_status, keep * sizeof *h_status);
    }
    gcn10_job_list_free(g, ctx, l);
    l->h_jobs = h_jobs;
    l->h_status = h_status;
    /* (the capacity stays 0 until all five are there) */
    if ((rc = g->malloc(ctx, n * sizeof *l->d_jobs, (void **)&l->d_jobs)) != 0 ||
        (rc = g->malloc(ctx, n * sizeof *l->d_status, (void **)&l->d_status)) != 0 ||
        (rc = g->host_alloc(ctx, n * sizeof *l->bad, (void **)&l->bad)) != 0)
        return rc;
    l->cap = n;
    return 0;
}

/* ------------------------------------------------------------------------ */
/* the ring                                                                  */
/* ------------------------------------------------------------------------ */

int gcn10_stager_setup(struct gcn10_stager *s, const struct gcn10_gpu_api *g, gcn10_gpu_ctx *ctx, gcn10_pool *pool,
                       atomic_llong *pinned_bytes, int n_buffers, size_t bytes)
{
    int rc;

    memset(s, 0, sizeof *s);
    s->gpu = g;
    s->ctx = ctx;
    s->pool = pool;
    s->pinned_bytes = pinned_bytes;
    s->n = n_buffers;
    gcn10_job_group_init(&s->reads);
    for (int k = 0; k < s->n; k++)
        if ((rc = g->event_create(ctx, &s->ev[k])) != 0)
            return rc;
    return gcn10_stager_ensure(s, bytes);
}

void gcn10_stager_teardown(struct gcn10_stager *s)
{
    if (!s->gpu)
        return;                         /* never set up */
    for (int k = 0; k < s->n; k++) {
        if (s->h[k]) s->gpu->host_free(s->ctx, s->h[k]);
        if (s->ev[k]) s->gpu->event_destroy(s->ctx, s->ev[k]);
    }
    gcn10_job_group_destroy(&s->reads);
    memset(s, 0, sizeof *s);
}

int gcn10_stager_take(struct gcn10_stager *s, int k)
{
    if (s->busy[k]) {
        const int rc = s->gpu->event_sync(s->ctx, s->ev[k]);

        if (rc != 0)
            return rc;
        s->busy[k] = false;
    }
    return 0;
}

int gcn10_stager_sent(struct gcn10_stager *s, int k, gcn10_stream_t stream)
{
    const int rc = s->gpu->event_record(s->ctx, s->ev[k], stream);

    if (rc == 0)
        s->busy[k] = true;
    return rc;
}

void gcn10_stager_idle(struct gcn10_stager *s)
{
    for (int k = 0; k < s->n; k++)
        s->busy[k] = false;
}

int gcn10_stager_ensure(struct gcn10_stager *s, size_t bytes)
{
    int rc;

    if (bytes <= s->cap)
        return 0;
    for (int k = 0; k < s->n; k++) {
        if ((rc = gcn10_stager_take(s, k)) != 0)
            return rc;
        if (s->h[k])
            s->gpu->host_free(s->ctx, s->h[k]);
        s->h[k] = NULL;
    }
    s->cap = 0;
    bytes = (bytes + 4095) & ~(size_t)4095;
    for (int k = 0; k < s->n; k++) {
        if ((rc = s->gpu->host_alloc(s->ctx, bytes, (void **)&s->h[k])) != 0)
            return rc;
        atomic_fetch_add(s->pinned_bytes, (long long)bytes);
    }
    s->cap = bytes;
    return 0;
}

/* ------------------------------------------------------------------------ */
/* chunks -> ring -> device                                                  */
/* ------------------------------------------------------------------------ */

/* One pool job: the next SLICE chunks of the batch, each to dst + (in_off - base).  Every job of a batch gets the
 * stager itself as its argument and takes its slice here, so a job needs no memory of its own. */
static void read_slice(void *arg)
{
    struct gcn10_stager *s = arg;
    const size_t i0 = atomic_fetch_add(&s->next, SLICE), i1 = s->end - i0 < SLICE ? s->end : i0 + SLICE;

    for (size_t i = i0; i < i1; i++) {
        uint8_t *const p0 = s->dst + (s->jobs[i].in_off - s->base), *p = p0;
        size_t left = s->chunks[i].nbytes;
        uint64_t off = s->chunks[i].file_off;

        while (left > 0) {
            const ssize_t got = pread(s->chunks[i].fd, p, left, (off_t)off);

            if (got <= 0) {
                s->bad[i] = 1;
                p = p0 + s->chunks[i].nbytes;
                memset(p0, 0, s->chunks[i].nbytes);     /* nothing of a chunk that is not whole */
                break;
            }
            p += got;
            off += (uint64_t)got;
            left -= (size_t)got;
        }
        memset(p, 0, 16);               /* the decoder's bit reader may look a few bytes ahead */
    }
    gcn10_job_group_done(&s->reads);
}

int gcn10_stager_stage(struct gcn10_stager *s, const struct gcn10_chunk_ref *chunks, const gcn10_inflate_tile *jobs,
                       size_t n, uint8_t *d_comp, gcn10_stream_t stream, int *bad)
{
    int rc, k = 0;

    for (size_t i = 0; i < n; i++)
        bad[i] = 0;
    for (size_t i0 = 0; i0 < n;) {
        const uint64_t base = jobs[i0].in_off;
        uint64_t end = base;
        size_t i1 = i0;
        int n_slices;

        while (i1 < n) {
            const uint64_t e = jobs[i1].in_off + gcn10_chunk_slot(jobs[i1].in_len);

            if (e - base > s->cap)
                break;
            end = e;
            i1++;
        }
        if (i1 == i0) {
            bad[i0++] = 2;              /* one chunk larger than a buffer */
            continue;
        }
        if ((rc = gcn10_stager_take(s, k)) != 0)
            return rc;
        n_slices = (int)((i1 - i0 + SLICE - 1) / SLICE);
        s->chunks = chunks;
        s->jobs = jobs;
        s->bad = bad;
        s->dst = s->h[k];
        s->base = base;
        atomic_store(&s->next, i0);
        s->end = i1;
        gcn10_job_group_add(&s->reads, n_slices);
        for (int j = 0; j < n_slices; j++) {
            if (s->pool)
                gcn10_pool_submit(s->pool, read_slice, s);
            else
                read_slice(s);
        }
        gcn10_job_group_wait(&s->reads);
        if ((rc = s->gpu->memcpy_h2d(s->ctx, d_comp + base, s->h[k], (size_t)(end - base), stream)) != 0 ||
            (rc = gcn10_stager_sent(s, k, stream)) != 0)
            return rc;
        k = (k + 1) % s->n;
        i0 = i1;
    }
    return 0;
}
