/* tiff_cache.c -- decoded chunks that windows use a small part of.  (The module as a whole: tiff_internal.h.)
 *
 * The soil raster is a global file of full-width strips: a block's window needs 1/120 of each strip it touches, and
 * the ~120 blocks of a latitude band need the SAME strips, one block after the other (the queue hands out ids in
 * shapefile order).  Decoding a strip once per block was the largest item of the host's CPU time without the file
 * sink (profiles/r03/host_cpu_by_thread_and_job.txt).  One cache per process, shared by every handle of a file
 * (workers open their own), least recently used out first; GCN10_CHUNK_CACHE_MB (default 512, 0 = none).  Entries in
 * use (being copied from) are not evicted.
 */
#include "tiff_internal.h"

#include <pthread.h>
#include <stdlib.h>

static struct {
    pthread_mutex_t mu;
    struct gcn10_cache_entry **e;   /* heap objects: a pinned entry is referred to by pointer while others come and go */
    int n, cap_entries;
    size_t bytes, cap_bytes;
    uint64_t clock, hits, misses;
    bool ready;
} g_cache = { .mu = PTHREAD_MUTEX_INITIALIZER };

static void cache_init_locked(void)
{
    const char *mb = getenv("GCN10_CHUNK_CACHE_MB");

    g_cache.cap_bytes = (size_t)(mb ? strtoull(mb, NULL, 10) : 512) << 20;
    g_cache.ready = true;
}

/* the entry of that chunk, pinned, or NULL; the lock is held */
static struct gcn10_cache_entry *find_and_pin_locked(const struct gcn10_tiff *t, uint64_t idx, size_t bytes)
{
    for (int i = 0; i < g_cache.n; i++) {
        struct gcn10_cache_entry *c = g_cache.e[i];

        if (c->idx == idx && c->ino == t->id_ino && c->dev == t->id_dev && c->bytes == bytes) {
            c->refs++;
            return c;
        }
    }
    return NULL;
}

struct gcn10_cache_entry *gcn10_chunk_cache_get(const struct gcn10_tiff *t, uint64_t idx, size_t bytes)
{
    struct gcn10_cache_entry *hit;

    pthread_mutex_lock(&g_cache.mu);
    if (!g_cache.ready)
        cache_init_locked();
    hit = find_and_pin_locked(t, idx, bytes);
    if (hit) {
        hit->stamp = ++g_cache.clock;
        g_cache.hits++;
    }
    else {
        g_cache.misses++;
    }
    pthread_mutex_unlock(&g_cache.mu);
    return hit;
}

void gcn10_chunk_cache_release(struct gcn10_cache_entry *c)
{
    pthread_mutex_lock(&g_cache.mu);
    c->refs--;
    pthread_mutex_unlock(&g_cache.mu);
}

struct gcn10_cache_entry *gcn10_chunk_cache_put(const struct gcn10_tiff *t, uint64_t idx, unsigned char *data,
                                                size_t bytes)
{
    struct gcn10_cache_entry *res = NULL;

    pthread_mutex_lock(&g_cache.mu);
    if (bytes <= g_cache.cap_bytes / 4) {
        res = find_and_pin_locked(t, idx, bytes);
        if (res) {                                  /* decoded by another thread meanwhile: use theirs */
            pthread_mutex_unlock(&g_cache.mu);
            free(data);
            return res;
        }
        while (g_cache.bytes + bytes > g_cache.cap_bytes) {      /* least recently used, not in use, out */
            int victim = -1;

            for (int i = 0; i < g_cache.n; i++)
                if (g_cache.e[i]->refs == 0 && (victim < 0 || g_cache.e[i]->stamp < g_cache.e[victim]->stamp))
                    victim = i;
            if (victim < 0)
                break;
            g_cache.bytes -= g_cache.e[victim]->bytes;
            free(g_cache.e[victim]->data);
            free(g_cache.e[victim]);
            g_cache.e[victim] = g_cache.e[--g_cache.n];
        }
        if (g_cache.bytes + bytes <= g_cache.cap_bytes) {
            if (g_cache.n == g_cache.cap_entries) {
                int cap = g_cache.cap_entries ? g_cache.cap_entries * 2 : 4096;
                struct gcn10_cache_entry **g = realloc(g_cache.e, (size_t)cap * sizeof *g);

                if (g) {
                    g_cache.e = g;
                    g_cache.cap_entries = cap;
                }
            }
            if (g_cache.n < g_cache.cap_entries && (res = malloc(sizeof *res)) != NULL) {
                *res = (struct gcn10_cache_entry){ t->id_dev, t->id_ino, idx, data, bytes, ++g_cache.clock, 1 };
                g_cache.e[g_cache.n++] = res;
                g_cache.bytes += bytes;
            }
        }
    }
    pthread_mutex_unlock(&g_cache.mu);
    return res;
}

bool gcn10_chunk_cache_enabled(void)
{
    bool on;

    pthread_mutex_lock(&g_cache.mu);
    if (!g_cache.ready)
        cache_init_locked();
    on = g_cache.cap_bytes > 0;
    pthread_mutex_unlock(&g_cache.mu);
    return on;
}

void gcn10_tiff_cache_stats(uint64_t *hits, uint64_t *misses, size_t *bytes)
{
    pthread_mutex_lock(&g_cache.mu);
    if (hits)
        *hits = g_cache.hits;
    if (misses)
        *misses = g_cache.misses;
    if (bytes)
        *bytes = g_cache.bytes;
    pthread_mutex_unlock(&g_cache.mu);
}
