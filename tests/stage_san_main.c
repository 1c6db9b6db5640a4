/* stage_san_main.c -- stand-alone driver of the chunk stager (gcn10_amd/csrc/host/stage.c, with pool.c), built by
 * tests/test_stage_host.py with -fsanitize=address,undefined.
 *
 *   stage_san <directory>
 *
 * Stages chunks of a file it writes into the directory through a stager of 2 buffers x 4 KiB, with and without an I/O
 * pool, into a host stand-in for device memory, and checks every byte that arrives.  The GPU library is a table of host
 * fakes.  A copy "to the device" is only queued when it is issued and carried out when its event -- or the whole
 * stream -- is waited for, as late as a real copy may happen: a buffer written again, or freed, before the stager has
 * waited for its event shows as wrong bytes or as a sanitizer report.  Prints "stage_san: N cases ok" (exit 0), or the
 * first failed check (exit 1). */
#include "pipeline_internal.h"

#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

enum { FILE_BYTES = 1 << 16, BUF = 4096, FILL = 0xEE, MAX_CHUNKS = 128 };

/* ---- the fakes ---- */

struct copy { void *dst; const void *src; size_t n; };
static struct copy queue[1024];
static size_t q_len, q_done;
static long n_copies;

static void run_copies(size_t upto)
{
    for (; q_done < upto; q_done++)
        memcpy(queue[q_done].dst, queue[q_done].src, queue[q_done].n);
}

static int f_malloc(gcn10_gpu_ctx *c, size_t n, void **p)
{
    (void)c;
    *p = malloc(n ? n : 1);
    if (*p)
        memset(*p, FILL, n);
    return *p ? 0 : -1;
}

static int f_free(gcn10_gpu_ctx *c, void *p)
{
    (void)c;
    free(p);
    return 0;
}

static int f_h2d(gcn10_gpu_ctx *c, void *dst, const void *src, size_t n, gcn10_stream_t s)
{
    (void)c;
    (void)s;
    if (q_len == sizeof queue / sizeof queue[0]) {
        fprintf(stderr, "stage_san: copy queue full\n");
        exit(1);
    }
    queue[q_len++] = (struct copy){ dst, src, n };
    n_copies++;
    return 0;
}

static int f_event_create(gcn10_gpu_ctx *c, gcn10_event_t *e)
{
    (void)c;
    *e = calloc(1, sizeof(size_t));
    return *e ? 0 : -1;
}

static int f_event_destroy(gcn10_gpu_ctx *c, gcn10_event_t e)
{
    (void)c;
    free(e);
    return 0;
}

static int f_event_record(gcn10_gpu_ctx *c, gcn10_event_t e, gcn10_stream_t s)
{
    (void)c;
    (void)s;
    *(size_t *)e = q_len;
    return 0;
}

static int f_event_sync(gcn10_gpu_ctx *c, gcn10_event_t e)
{
    (void)c;
    run_copies(*(size_t *)e);
    return 0;
}

static const char *f_last_error(void)
{
    return "fake";
}

static const struct gcn10_gpu_api fake = {
    .loaded = true, .last_error = f_last_error, .malloc = f_malloc, .free = f_free, .host_alloc = f_malloc,
    .host_free = f_free, .memcpy_h2d = f_h2d, .event_create = f_event_create, .event_destroy = f_event_destroy,
    .event_record = f_event_record, .event_sync = f_event_sync,
};

/* ---- one call of gcn10_stager_stage, checked ---- */

static uint8_t file_bytes[FILE_BYTES];
static int n_cases;

#define CHECK(cond, ...)                                    \
    do {                                                    \
        if (!(cond)) {                                      \
            fprintf(stderr, "stage_san: %s: ", name);       \
            fprintf(stderr, __VA_ARGS__);                   \
            fprintf(stderr, "\n");                          \
            exit(1);                                        \
        }                                                   \
    } while (0)

/* chunk i: c[i].nbytes bytes at c[i].file_off of c[i].fd; want[i]: the bad[] value it must get; copies: how many
 * copies to the device the call must make (-1: any number) */
static void stage_and_check(const char *name, struct gcn10_stager *s, struct gcn10_chunk_ref *c, const int *want,
                            size_t n, long copies)
{
    static gcn10_inflate_tile jobs[MAX_CHUNKS];
    static int bad[MAX_CHUNKS];
    size_t total = 0;
    uint8_t *d_comp;
    const long copies0 = n_copies;

    for (size_t i = 0; i < n; i++) {
        c[i].out_len = c[i].nbytes;
        c[i].flags = GCN10_TILE_RAW;
        gcn10_inflate_job_from_chunk(&jobs[i], &c[i], total, 0);
        CHECK(jobs[i].in_off == total && jobs[i].in_len == c[i].nbytes, "job %zu is not its chunk", i);
        total += gcn10_chunk_slot(c[i].nbytes);
        bad[i] = 77;
    }
    d_comp = malloc(total + 16);
    CHECK(d_comp, "malloc");
    memset(d_comp, FILL, total + 16);
    CHECK(gcn10_stager_stage(s, c, jobs, n, d_comp, NULL, bad) == 0, "the call failed");
    CHECK(copies < 0 || n_copies - copies0 == copies, "%ld copies, not %ld", n_copies - copies0, copies);
    run_copies(q_len);                  /* the caller waits for the stream ... */
    gcn10_stager_idle(s);               /* ... and says so */
    for (size_t i = 0; i < n; i++) {
        const uint8_t *p = d_comp + jobs[i].in_off;
        const size_t slot = gcn10_chunk_slot(c[i].nbytes);

        CHECK(bad[i] == want[i], "chunk %zu of %u bytes: bad %d, not %d", i, c[i].nbytes, bad[i], want[i]);
        for (size_t b = 0; b < slot; b++) {
            /* staged: the file's bytes, then 16 zeros (and what aligns the next chunk is anything); unreadable: zeros
             * in their place; too large: nothing */
            const int v = want[i] == 2 ? FILL : (b >= c[i].nbytes || want[i] == 1 ? 0 : file_bytes[c[i].file_off + b]);

            if (want[i] != 2 && b >= (size_t)c[i].nbytes + 16)
                break;
            CHECK(p[b] == v, "chunk %zu of %u bytes (bad %d): byte %zu is %u, not %d", i, c[i].nbytes, want[i], b, p[b], v);
        }
    }
    CHECK(d_comp[total] == FILL, "a byte behind the last chunk was written");
    free(d_comp);
    n_cases++;
}

/* chunks of the given sizes, one after the other in the file */
static size_t lay_out(struct gcn10_chunk_ref *c, int *want, int fd, const uint32_t *sizes, size_t n)
{
    uint64_t off = 3;

    memset(c, 0, n * sizeof *c);
    for (size_t i = 0; i < n; i++) {
        c[i].fd = fd;
        c[i].file_off = off;
        c[i].nbytes = sizes[i];
        off += sizes[i];
        want[i] = 0;
    }
    return n;
}

static void all_cases(const char *name, int fd, int closed_fd, gcn10_pool *pool)
{
    static struct gcn10_chunk_ref c[MAX_CHUNKS];
    static int want[MAX_CHUNKS];
    atomic_llong pinned = 0;
    struct gcn10_stager s;
    uint32_t sizes[MAX_CHUNKS];
    size_t n;

    CHECK(gcn10_stager_setup(&s, &fake, NULL, pool, &pinned, 2, BUF) == 0, "setup");
    CHECK(s.cap == BUF && atomic_load(&pinned) == 2 * BUF, "2 buffers of %d bytes expected", BUF);

    stage_and_check(name, &s, c, want, 0, 0);                                   /* no chunk */
    n = lay_out(c, want, fd, (uint32_t[]){ 100 }, 1);                           /* one */
    stage_and_check(name, &s, c, want, n, 1);
    n = lay_out(c, want, fd, (uint32_t[]){ 1008, 1008, 1008, 1008 }, 4);        /* 4 x 1024: exactly one buffer */
    stage_and_check(name, &s, c, want, n, 1);
    n = lay_out(c, want, fd, (uint32_t[]){ 1008, 1008, 1008, 1009 }, 4);        /* one byte more: a second one */
    stage_and_check(name, &s, c, want, n, 2);
    n = lay_out(c, want, fd, (uint32_t[]){ 1008, 1008, 1008, 1008, 1008, 1008, 1008, 1008, 1008 }, 9);  /* the ring turns */
    stage_and_check(name, &s, c, want, n, 3);
    for (int i = 0; i < 100; i++)                                               /* 100 of mixed sizes, empty ones too; */
        sizes[i] = (uint32_t)((i * 37) % 60 + (i % 25 == 24 ? 900 : 0));         /* ~49 per buffer: two pool jobs each */
    n = lay_out(c, want, fd, sizes, 100);
    stage_and_check(name, &s, c, want, n, -1);
    n = lay_out(c, want, fd, (uint32_t[]){ 500, BUF - 16, 500 }, 3);            /* a slot of exactly one buffer */
    stage_and_check(name, &s, c, want, n, 3);
    n = lay_out(c, want, fd, (uint32_t[]){ 500, BUF - 15, 500, 20 }, 4);        /* one byte larger: not staged */
    want[1] = 2;
    stage_and_check(name, &s, c, want, n, 2);
    n = lay_out(c, want, fd, (uint32_t[]){ 300, 400, 500, 600, 700 }, 5);       /* ends beyond the end of the file; */
    c[1].file_off = FILE_BYTES - 399;
    want[1] = 1;
    c[3].fd = closed_fd;                                                        /* a closed descriptor; */
    want[3] = 1;
    c[4].file_off = FILE_BYTES;                                                 /* starts at the end of the file */
    want[4] = 1;
    stage_and_check(name, &s, c, want, n, 1);

    /* the ring grows between two calls, while copies out of its old buffers are still due */
    n = lay_out(c, want, fd, (uint32_t[]){ 3000, 3000, 3000 }, 3);
    {
        gcn10_inflate_tile jobs[3];
        int bad[3];
        uint8_t *d = malloc(3 * 3024);

        CHECK(d, "malloc");
        for (size_t i = 0; i < 3; i++)
            gcn10_inflate_job_from_chunk(&jobs[i], &c[i], i * 3024, 0);
        CHECK(gcn10_stager_stage(&s, c, jobs, 3, d, NULL, bad) == 0, "the call failed");
        CHECK(gcn10_stager_ensure(&s, 100) == 0 && s.cap == BUF, "a smaller size must change nothing");
        CHECK(gcn10_stager_ensure(&s, 2 * BUF - 100) == 0 && s.cap == 2 * BUF, "growth to %d bytes", 2 * BUF);
        CHECK(atomic_load(&pinned) == 2 * BUF + 4 * BUF, "pinned bytes counted: %lld", atomic_load(&pinned));
        run_copies(q_len);
        for (size_t i = 0; i < 3; i++)
            CHECK(memcmp(d + i * 3024, file_bytes + c[i].file_off, 3000) == 0, "chunk %zu lost while the ring grew", i);
        free(d);
        n_cases++;
    }
    n = lay_out(c, want, fd, (uint32_t[]){ 6000, BUF - 15, 2 * BUF - 16, 2 * BUF - 15 }, 4);
    want[3] = 2;
    stage_and_check(name, &s, c, want, n, 3);
    gcn10_stager_teardown(&s);
    gcn10_stager_teardown(&s);          /* (one that is not set up: nothing) */
}

static void job_list_case(void)
{
    const char *name = "job list";
    struct gcn10_job_list l = { 0 };

    CHECK(gcn10_job_list_ensure(&fake, NULL, &l, 0, 0) == 0 && l.cap == 0, "room for nothing");
    CHECK(gcn10_job_list_ensure(&fake, NULL, &l, 4, 0) == 0 && l.cap == 4, "room for 4");
    for (uint32_t i = 0; i < 4; i++) {
        l.h_jobs[i].in_len = 1000 + i;
        l.h_status[i] = 2000 + i;
    }
    CHECK(gcn10_job_list_ensure(&fake, NULL, &l, 3, 0) == 0 && l.cap == 4, "no growth for less");
    CHECK(gcn10_job_list_ensure(&fake, NULL, &l, 50, 4) == 0 && l.cap == 50 && l.d_jobs && l.d_status, "room for 50");
    for (uint32_t i = 0; i < 4; i++)
        CHECK(l.h_jobs[i].in_len == 1000 + i && l.h_status[i] == 2000 + i, "entry %u not kept", i);
    l.h_jobs[49].in_len = 1;
    l.h_status[49] = 1;
    gcn10_job_list_free(&fake, NULL, &l);
    CHECK(!l.h_jobs && !l.d_jobs && !l.h_status && !l.d_status && l.cap == 0, "freed");
    n_cases++;
}

int main(int argc, char **argv)
{
    const char *name = "setup";
    char path[4096];
    gcn10_pool *pool;
    int fd, closed_fd;

    if (argc != 2) {
        fprintf(stderr, "usage: stage_san <directory>\n");
        return 2;
    }
    for (size_t i = 0; i < FILE_BYTES; i++)
        file_bytes[i] = (uint8_t)(1 + (i * 2654435761u >> 11) % 255);       /* never 0: a zero that arrives was put there */
    snprintf(path, sizeof path, "%s/chunks.bin", argv[1]);
    fd = open(path, O_CREAT | O_TRUNC | O_RDWR, 0600);
    CHECK(fd >= 0 && write(fd, file_bytes, FILE_BYTES) == FILE_BYTES, "cannot write %s", path);
    closed_fd = 1 << 20;                /* a number no open descriptor of this process has, now or later */
    CHECK(fcntl(closed_fd, F_GETFD) == -1, "descriptor %d is open", closed_fd);

    CHECK(gcn10_chunk_slot(0) == 16 && gcn10_chunk_slot(1) == 32 && gcn10_chunk_slot(16) == 32 &&
          gcn10_chunk_slot(17) == 48 && gcn10_chunk_slot(0xffffffffu) == 0x100000010ull, "slot sizes");
    job_list_case();
    all_cases("no pool", fd, closed_fd, NULL);
    pool = gcn10_pool_create(4);
    CHECK(pool, "pool");
    all_cases("pool of 4", fd, closed_fd, pool);
    gcn10_pool_destroy(pool);
    close(fd);
    printf("stage_san: %d cases ok\n", n_cases);
    return 0;
}
