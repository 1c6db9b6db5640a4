/* tiff_write.c -- the tiled GeoTIFF writer: tiles arrive compressed and are appended (one pwrite, gathered writes, or
 * one aligned write of an extent, with or without direct I/O); the directories follow at the end (a plain file) or
 * lie in room kept for them at the front (a Cloud Optimized GeoTIFF, with one directory per overview level), carrying
 * the georeferencing and the GDAL_NODATA / GDAL_METADATA tags; gcn10_deflate_tile and gcn10_save_raster on top.
 * (The module as a whole: tiff_internal.h.)
 */
#include "tiff_internal.h"

#include <errno.h>
#include <fcntl.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/uio.h>
#include <unistd.h>
#include <zlib.h>

enum { TILE = 256 };        /* GDAL's default block size for TILED=YES */

struct gcn10_tiff_writer {
    int fd;
    char *path;
    char *part;                 /* the file is written under this name and renamed when complete */
    int xsize, ysize, across, down;
    double gt[6];
    gcn10_georef georef;        /* deep copy */
    uint32_t *offsets, *counts;
    uint64_t pos;               /* append position */
    pthread_mutex_t mu;
    bool failed;
    bool direct;                /* O_DIRECT is set on fd: extents go out at 4096-aligned positions */
    int compression;            /* TIFF Compression tag: 8 (Adobe deflate, default) or 5 (LZW) */
    /* Cloud Optimized GeoTIFF layout (gcn10_tiff_create_cog).  A COG writer owns one view per overview
     * level; a view has its own size and tile arrays and shares the file (fd, pos, mu, failed, direct) with
     * its root.  A plain writer is its own root with no levels. */
    struct gcn10_tiff_writer *root;
    struct gcn10_tiff_writer **levels;  /* root of a COG: views of levels 1 .. n_levels, [k - 1] */
    int n_levels, level;
    bool cog;
    int cur_level;              /* root of a COG: the level tile data goes to now (starts at n_levels) */
    long long last_idx;         /* COG: highest tile index of this level written so far (-1: none) */
    uint64_t data_start;        /* root of a COG: first byte after the IFDs, where tile data begins */
    /* GDAL tags of the root (gcn10_tiff_set_nodata, gcn10_tiff_set_metadata_xml) */
    int nodata;                 /* -1: no GDAL_NODATA tag */
    char nodata_s[4];           /* its ASCII value, e.g. "255" */
    char *metadata;             /* GDAL_METADATA text of the full-resolution IFD, or NULL */
    size_t metadata_room;       /* COG: bytes reserved for it (0: none; the tag is then written only with a text) */
};

static int write_all(int fd, const void *buf, size_t n, uint64_t off)
{
    const unsigned char *p = buf;

    while (n) {
        ssize_t w = pwrite(fd, p, n, (off_t)off);

        if (w < 0 && errno == EINTR)
            continue;
        if (w <= 0)
            return -1;
        p += w;
        off += (uint64_t)w;
        n -= (size_t)w;
    }
    return 0;
}

static void free_georef(gcn10_georef *g)
{
    free(g->geokeys);
    free(g->geodoubles);
    free(g->geoascii);
    memset(g, 0, sizeof *g);
}

static int copy_georef(gcn10_georef *dst, const gcn10_georef *src)
{
    /* default: EPSG:4326 geographic, pixel-is-area -- what both inputs of this
     * program are (README of the reference: "HYSOGs250m_4326", WorldCover) */
    static const uint16_t wgs84[] = { 1, 1, 0, 3, 1024, 0, 1, 2, 1025, 0, 1, 1, 2048, 0, 1, 4326 };

    memset(dst, 0, sizeof *dst);
    if (!src || !src->geokeys || src->n_geokeys < 4) {
        dst->geokeys = malloc(sizeof wgs84);
        if (!dst->geokeys)
            return -1;
        memcpy(dst->geokeys, wgs84, sizeof wgs84);
        dst->n_geokeys = (int)(sizeof wgs84 / sizeof wgs84[0]);
        return 0;
    }
    dst->geokeys = malloc((size_t)src->n_geokeys * sizeof(uint16_t));
    if (!dst->geokeys)
        return -1;
    memcpy(dst->geokeys, src->geokeys, (size_t)src->n_geokeys * sizeof(uint16_t));
    dst->n_geokeys = src->n_geokeys;
    if (src->geodoubles && src->n_geodoubles > 0) {
        dst->geodoubles = malloc((size_t)src->n_geodoubles * sizeof(double));
        if (!dst->geodoubles)
            return -1;
        memcpy(dst->geodoubles, src->geodoubles, (size_t)src->n_geodoubles * sizeof(double));
        dst->n_geodoubles = src->n_geodoubles;
    }
    if (src->geoascii) {
        dst->geoascii = strdup(src->geoascii);
        if (!dst->geoascii)
            return -1;
    }
    return 0;
}

int gcn10_tiff_set_compression(gcn10_tiff_writer *w, int compression)
{
    if (compression != 8 && compression != 5)
        return -1;
    w->root->compression = compression;     /* every IFD of a COG has the same Compression */
    return 0;
}

/* what the root and every level view have of their own: a size and one offset and one count per tile; 0 or -1 */
static int init_size_and_tiles(gcn10_tiff_writer *v, int xsize, int ysize)
{
    v->fd = -1;
    v->last_idx = -1;
    v->xsize = xsize;
    v->ysize = ysize;
    v->across = (xsize + TILE - 1) / TILE;
    v->down = (ysize + TILE - 1) / TILE;
    v->offsets = calloc((size_t)v->across * (size_t)v->down, sizeof *v->offsets);
    v->counts = calloc((size_t)v->across * (size_t)v->down, sizeof *v->counts);
    return v->offsets && v->counts ? 0 : -1;
}

gcn10_tiff_writer *gcn10_tiff_create(const char *path, int xsize, int ysize, const double gt[6],
                                     const gcn10_georef *georef, char *err, size_t errcap)
{
    static const unsigned char header[8] = { 'I', 'I', 42, 0, 0, 0, 0, 0 };
    gcn10_tiff_writer *w;
    int sized;

    if (xsize <= 0 || ysize <= 0) {
        snprintf(err, errcap, "write error: bad raster size %dx%d for %s", xsize, ysize, path);
        return NULL;
    }
    w = calloc(1, sizeof *w);
    if (!w)
        goto oom;
    w->compression = 8;
    w->nodata = -1;
    w->root = w;
    pthread_mutex_init(&w->mu, NULL);
    sized = init_size_and_tiles(w, xsize, ysize);
    memcpy(w->gt, gt, sizeof w->gt);
    w->path = strdup(path);
    w->part = malloc(strlen(path) + 6);
    if (w->part)
        sprintf(w->part, "%s.part", path);
    if (sized != 0 || !w->path || !w->part || copy_georef(&w->georef, georef) != 0)
        goto oom;
    /* an existing raster of that name stays as it is until this one is complete */
    w->fd = open(w->part, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (w->fd < 0 || write_all(w->fd, header, sizeof header, 0) != 0) {
        snprintf(err, errcap, "write error: cannot create %s: %s", path, strerror(errno));
        gcn10_tiff_abort(w);
        return NULL;
    }
    w->pos = sizeof header;
    return w;

oom:
    snprintf(err, errcap, "out of memory creating %s", path);
    if (w)
        gcn10_tiff_abort(w);
    return NULL;
}

int gcn10_tiff_tiles_across(const gcn10_tiff_writer *w)
{
    return w->across;
}

int gcn10_tiff_tiles_down(const gcn10_tiff_writer *w)
{
    return w->down;
}

int gcn10_cog_levels(int xsize, int ysize)
{
    int k = 0;

    if (xsize <= 0 || ysize <= 0)
        return -1;
    while (xsize > TILE || ysize > TILE) {
        xsize = (xsize + 1) / 2;        /* ceil(W / 2^k) step by step: ceil(ceil(a/2)/2) = ceil(a/4) */
        ysize = (ysize + 1) / 2;
        k++;
    }
    return k;
}

static int cog_layout(gcn10_tiff_writer *R, int fd, uint64_t *first, uint64_t *end);

gcn10_tiff_writer *gcn10_tiff_create_cog(const char *path, int xsize, int ysize, const double gt[6],
                                         const gcn10_georef *georef, int n_levels, char *err, size_t errcap)
{
    gcn10_tiff_writer *w;
    uint64_t first, end;

    if (n_levels < 0 || n_levels > 30 || xsize <= 0 || ysize <= 0) {
        snprintf(err, errcap, "write error: bad overview level count %d for %dx%d (%s)", n_levels, xsize, ysize, path);
        return NULL;
    }
    w = gcn10_tiff_create(path, xsize, ysize, gt, georef, err, errcap);
    if (!w)
        return NULL;
    w->cog = true;
    w->n_levels = n_levels;
    w->cur_level = n_levels;
    w->levels = calloc(n_levels > 0 ? (size_t)n_levels : 1, sizeof *w->levels);
    if (!w->levels)
        goto oom;
    for (int k = 1; k <= n_levels; k++) {
        gcn10_tiff_writer *v = calloc(1, sizeof *v);

        if (!v)
            goto oom;
        w->levels[k - 1] = v;
        v->root = w;
        v->level = k;
        if (init_size_and_tiles(v, gcn10_level_dim(xsize, k), gcn10_level_dim(ysize, k)) != 0)
            goto oom;
    }
    /* the IFDs' room: their sizes depend only on the level sizes and the georeferencing */
    if (cog_layout(w, -1, &first, &end) != 0) {
        snprintf(err, errcap, "write error: directories of %s do not fit classic TIFF", path);
        gcn10_tiff_abort(w);
        return NULL;
    }
    w->data_start = end;
    w->pos = end;
    return w;

oom:
    snprintf(err, errcap, "out of memory creating %s", path);
    gcn10_tiff_abort(w);
    return NULL;
}

int gcn10_tiff_n_levels(const gcn10_tiff_writer *w)
{
    return w->root->n_levels;
}

gcn10_tiff_writer *gcn10_tiff_level(gcn10_tiff_writer *w, int level)
{
    w = w->root;
    if (level == 0)
        return w;
    if (level < 0 || level > w->n_levels)
        return NULL;
    return w->levels[level - 1];
}

/* ------------------------------------------------------------------------ */
/* tile puts                                                                 */
/* ------------------------------------------------------------------------ */

/* The three puts differ in how the bytes reach the file and in what a refusal costs; everything else is the four
 * routines below.  What a refusal costs, as it always was:
 *                                      put_tile        put_tiles               put_extent
 *   a tile outside the grid, 0 bytes   refused         writer failed (*)       refused
 *   streams outside the extent, or a
 *   COG's rel_off not increasing       --              --                      refused
 *   against a COG's order              refused         refused                 refused
 *   no room below 4 GiB                writer failed   writer failed           writer failed
 *   the write itself                   writer failed   writer failed           writer failed
 * "refused": -1 and the writer is as it was; "writer failed": -1 and gcn10_tiff_finish will answer "write error".
 * (*) put_tiles checks its tiles batch by batch behind the order rule, when earlier batches may have gone out; a
 * COG's order rule, which reads the coordinates first, turns a negative one into a plain refusal. */

static bool tile_in_grid(const gcn10_tiff_writer *w, int tx, int ty)
{
    return tx >= 0 && ty >= 0 && tx < w->across && ty < w->down;
}

/* classic TIFF offsets are 32 bit; a MiB is kept for the directories */
static bool room_up_to(uint64_t end)
{
    return end + (1u << 20) <= 0xffffffffull;
}

/* COG order rule (called with root->mu held): tile data is appended level L first, full resolution last, and in
 * each level in row-major tile order, so every IFD's offsets increase.  0 = the tiles idx[0..n) (ascending) may go
 * next; -1 = they would break the order.  Always 0 for a plain file. */
static int cog_order_ok(gcn10_tiff_writer *w, int n, const int *tx, const int *ty)
{
    long long prev = w->last_idx;

    if (!w->root->cog)
        return 0;
    if (w->level > w->root->cur_level)
        return -1;
    if (w->level < w->root->cur_level)
        prev = -1;                      /* the first put of a finer level */
    for (int i = 0; i < n; i++) {
        long long idx = (long long)ty[i] * w->across + tx[i];

        if (idx <= prev)
            return -1;
        prev = idx;
    }
    return 0;
}

/* The one place a put's tiles enter the directory (root->mu held, their bytes are in the file): stream i lies at
 * at + rel_off[i], or with rel_off == NULL the streams lie back to back from `at`; the append position moves to `end`
 * and a COG's order to the last tile. */
static void commit_tiles(gcn10_tiff_writer *w, int n, const int *tx, const int *ty, uint64_t at,
                         const uint32_t *rel_off, const uint32_t *nbytes, uint64_t end)
{
    gcn10_tiff_writer *R = w->root;

    for (int i = 0; i < n; i++) {
        const size_t idx = (size_t)ty[i] * (size_t)w->across + (size_t)tx[i];

        w->offsets[idx] = (uint32_t)(rel_off ? at + rel_off[i] : at);
        w->counts[idx] = nbytes[i];
        if (!rel_off)
            at += nbytes[i];
    }
    R->pos = end;
    if (R->cog && n > 0) {
        R->cur_level = w->level;
        w->last_idx = (long long)ty[n - 1] * w->across + tx[n - 1];
    }
}

/* A put_tile / put_tiles write goes at the append position with the streams' own lengths, neither of them sector
 * aligned, which ext4 and xfs refuse on an O_DIRECT descriptor (EINVAL).  So the file is written buffered from its
 * first such put on: same offsets and append position as a file that never had direct I/O.  R->mu is held. */
static void unaligned_put_ahead(gcn10_tiff_writer *R)
{
    if (R->direct)
        gcn10_tiff_set_direct(R, false);
}

int gcn10_tiff_put_tile(gcn10_tiff_writer *w, int tx, int ty, const void *zdata, size_t nbytes)
{
    gcn10_tiff_writer *R = w->root;
    const uint32_t len = (uint32_t)nbytes;
    int rc = -1;

    if (!tile_in_grid(w, tx, ty) || nbytes == 0)
        return -1;
    pthread_mutex_lock(&R->mu);
    if (cog_order_ok(w, 1, &tx, &ty) != 0) {
        /* refused; the file itself is still intact */
    }
    else if (!room_up_to(R->pos + nbytes)) {
        R->failed = true;
    }
    else {
        unaligned_put_ahead(R);
        if (R->direct || write_all(R->fd, zdata, nbytes, R->pos) != 0) {
            R->failed = true;           /* (R->direct: O_DIRECT could not be cleared) */
        }
        else {
            commit_tiles(w, 1, &tx, &ty, R->pos, NULL, &len, R->pos + nbytes);
            rc = 0;
        }
    }
    pthread_mutex_unlock(&R->mu);
    return rc;
}

/* m buffers to one file position, all of their bytes (pwritev may stop short); changes iov; 0 or -1 */
static int writev_all(int fd, struct iovec *iov, int m, uint64_t at)
{
    for (int k = 0; k < m;) {
        ssize_t got = pwritev(fd, iov + k, m - k, (off_t)at);

        if (got < 0 && errno == EINTR)
            continue;
        if (got <= 0)
            return -1;
        at += (uint64_t)got;
        while (k < m && (size_t)got >= iov[k].iov_len)
            got -= (ssize_t)iov[k++].iov_len;
        if (k < m && got > 0) {
            iov[k].iov_base = (char *)iov[k].iov_base + got;
            iov[k].iov_len -= (size_t)got;
        }
    }
    return 0;
}

/* Many tiles of one raster at once (a strip's worth from the GPU encoder): one pwritev per
 * 512 tiles instead of a pwrite per tile -- a block has 358 000 of them. */
int gcn10_tiff_put_tiles(gcn10_tiff_writer *w, int n, const int *tx, const int *ty, const void *const *zdata,
                         const uint32_t *nbytes)
{
    gcn10_tiff_writer *R = w->root;
    struct iovec iov[512];
    int rc = 0;

    pthread_mutex_lock(&R->mu);
    if (cog_order_ok(w, n, tx, ty) != 0) {
        pthread_mutex_unlock(&R->mu);
        return -1;
    }
    {
        /* a call that fails in a later batch leaves a COG's order where it was before the call */
        const long long last_idx = w->last_idx;
        const int cur_level = R->cur_level;

        unaligned_put_ahead(R);
        if (R->direct)
            rc = -1;                        /* O_DIRECT could not be cleared */
        for (int i = 0, m; i < n && rc == 0; i += m) {
            uint64_t total = 0;

            for (m = 0; i + m < n && m < 512; m++) {
                if (!tile_in_grid(w, tx[i + m], ty[i + m]) || nbytes[i + m] == 0) {
                    rc = -1;
                    break;
                }
                iov[m].iov_base = (void *)zdata[i + m];
                iov[m].iov_len = nbytes[i + m];
                total += nbytes[i + m];
            }
            if (rc != 0 || !room_up_to(R->pos + total) || writev_all(R->fd, iov, m, R->pos) != 0)
                rc = -1;
            else
                commit_tiles(w, m, tx + i, ty + i, R->pos, NULL, nbytes + i, R->pos + total);
        }
        if (rc != 0) {
            R->failed = true;
            w->last_idx = last_idx;
            R->cur_level = cur_level;
        }
    }
    pthread_mutex_unlock(&R->mu);
    return rc;
}

/* O_DIRECT for the tile data of this file (the directory is written without it at the end).  Extents
 * handed to gcn10_tiff_put_extent must then start at 4096-aligned addresses and be readable up to the
 * next multiple of 4096 past their end -- the pinned copy of the GPU encoder's arena is
 * (DIRECT_ALIGN = the encoder's "arena_segment_align").  A file system that refuses the flag leaves the
 * writer as it was: returns 0 when direct I/O is on, -1 when it is not. */
enum { DIRECT_ALIGN = 4096 };

int gcn10_tiff_set_direct(gcn10_tiff_writer *w, bool on)
{
    int fl;

    w = w->root;
    fl = fcntl(w->fd, F_GETFL);

    if (fl < 0)
        return -1;
    if (on == w->direct)
        return on ? 0 : -1;
#ifdef O_DIRECT
    if (fcntl(w->fd, F_SETFL, on ? (fl | O_DIRECT) : (fl & ~O_DIRECT)) != 0)
        return -1;
    w->direct = on;
    return on ? 0 : -1;
#else
    return -1;
#endif
}

/* n tiles of the raster whose streams lie in ONE extent of memory, `extent_bytes` long, stream i at
 * rel_off[i] (the layout the GPU encoders produce: a raster's streams of a strip back to back in tile order):
 * one write for all of them.  Same file contents as n gcn10_tiff_put_tile calls except for the few
 * alignment bytes between streams, which no directory entry points at. */
int gcn10_tiff_put_extent(gcn10_tiff_writer *w, const void *data, size_t extent_bytes, int n, const int *tx,
                          const int *ty, const uint32_t *rel_off, const uint32_t *nbytes)
{
    gcn10_tiff_writer *R = w->root;
    uint64_t at;
    size_t len = extent_bytes;
    int rc = 0;

    for (int i = 0; i < n; i++)
        if (!tile_in_grid(w, tx[i], ty[i]) || nbytes[i] == 0 ||
            (size_t)rel_off[i] + nbytes[i] > extent_bytes || (R->cog && i > 0 && rel_off[i] <= rel_off[i - 1]))
            return -1;
    pthread_mutex_lock(&R->mu);
    if (cog_order_ok(w, n, tx, ty) != 0) {
        pthread_mutex_unlock(&R->mu);
        return -1;
    }
    at = R->pos;
    if (R->direct) {
        at = (at + DIRECT_ALIGN - 1) / DIRECT_ALIGN * DIRECT_ALIGN;
        len = (len + DIRECT_ALIGN - 1) / DIRECT_ALIGN * DIRECT_ALIGN;
    }
    if (!room_up_to(at + len)) {
        rc = -1;
    }
    else if (write_all(R->fd, data, len, at) != 0) {
        if (R->direct && errno == EINVAL && gcn10_tiff_set_direct(R, false) != 0 && !R->direct) {
            /* this file system takes the flag and then refuses the write: once more without it */
            at = R->pos;
            len = extent_bytes;
            rc = write_all(R->fd, data, len, at) != 0 ? -1 : 0;
        }
        else {
            rc = -1;
        }
    }
    if (rc == 0)
        commit_tiles(w, n, tx, ty, at, rel_off, nbytes, at + len);
    else
        R->failed = true;
    pthread_mutex_unlock(&R->mu);
    return rc;
}

/* ------------------------------------------------------------------------ */
/* directories                                                               */
/* ------------------------------------------------------------------------ */

struct dirent_w {
    unsigned tag, type;
    uint32_t count;
    const void *data;       /* little-endian payload */
    size_t nbytes;
    size_t room;            /* file bytes kept for an out-of-line payload when more than nbytes (zero filled) */
};

/* the values the entries of one IFD point at */
struct ifd_vals {
    unsigned char s_sub[4], s_w[4], s_h[4], s_bps[2], s_comp[2], s_phot[2], s_spp[2], s_plan[2], s_tw[2], s_th[2],
        s_fmt[2];
    double scale[3], tie[6], xform[16];
};

/* Directory entries of level view v of root R, ascending tags.  v == R: the full-resolution IFD, the tag set of a
 * plain file; an overview level: NewSubfileType = 1 (reduced resolution), its own size and tiles, the same
 * Compression, no geo tags (readers take the georeferencing of overviews from the main IFD). */
static int ifd_entries(const gcn10_tiff_writer *R, const gcn10_tiff_writer *v, struct ifd_vals *x,
                       struct dirent_w ents[24])
{
    const size_t nt = (size_t)v->across * (size_t)v->down;
    int ne = 0;

    memset(x, 0, sizeof *x);
    x->scale[0] = R->gt[1];
    x->scale[1] = -R->gt[5];
    x->tie[3] = R->gt[0];
    x->tie[4] = R->gt[3];
    put32(x->s_sub, 1);
    put32(x->s_w, (uint32_t)v->xsize);
    put32(x->s_h, (uint32_t)v->ysize);
    put16(x->s_bps, 8);
    put16(x->s_comp, (unsigned)R->compression);     /* COMPRESS=DEFLATE -> Adobe deflate (8); COMPRESS=LZW -> 5 */
    put16(x->s_phot, 1);            /* MinIsBlack */
    put16(x->s_spp, 1);
    put16(x->s_plan, 1);
    put16(x->s_tw, TILE);
    put16(x->s_th, TILE);
    put16(x->s_fmt, 1);             /* unsigned integer */
#define ENT(tag_, type_, count_, data_, nbytes_) \
    ents[ne++] = (struct dirent_w){ tag_, type_, (uint32_t)(count_), data_, nbytes_, 0 }
    if (v != R)
        ENT(254, T_LONG, 1, x->s_sub, 4);
    ENT(256, T_LONG, 1, x->s_w, 4);
    ENT(257, T_LONG, 1, x->s_h, 4);
    ENT(258, T_SHORT, 1, x->s_bps, 2);
    ENT(259, T_SHORT, 1, x->s_comp, 2);
    ENT(262, T_SHORT, 1, x->s_phot, 2);
    ENT(277, T_SHORT, 1, x->s_spp, 2);
    ENT(284, T_SHORT, 1, x->s_plan, 2);
    ENT(322, T_SHORT, 1, x->s_tw, 2);
    ENT(323, T_SHORT, 1, x->s_th, 2);
    ENT(324, T_LONG, nt, v->offsets, nt * 4);      /* host is little endian (x86-64) */
    ENT(325, T_LONG, nt, v->counts, nt * 4);
    ENT(339, T_SHORT, 1, x->s_fmt, 2);
    if (v != R) {
        if (R->nodata >= 0)         /* GDAL writes GDAL_NODATA on the overview IFDs too */
            ENT(42113, T_ASCII, strlen(R->nodata_s) + 1, R->nodata_s, strlen(R->nodata_s) + 1);
        return ne;
    }
    if (R->gt[2] == 0.0 && R->gt[4] == 0.0) {
        ENT(33550, T_DOUBLE, 3, x->scale, sizeof x->scale);
        ENT(33922, T_DOUBLE, 6, x->tie, sizeof x->tie);
    }
    else {
        /* a rotated or sheared geotransform: ModelTransformationTag, the 4x4 matrix GDAL's
         * GTiff driver writes for GDALSetGeoTransform in that case (src/raster.c:210) */
        x->xform[0] = R->gt[1]; x->xform[1] = R->gt[2]; x->xform[3] = R->gt[0];
        x->xform[4] = R->gt[4]; x->xform[5] = R->gt[5]; x->xform[7] = R->gt[3];
        x->xform[15] = 1.0;
        ENT(34264, T_DOUBLE, 16, x->xform, sizeof x->xform);
    }
    if (R->georef.n_geokeys > 0 && R->georef.geokeys)
        ENT(34735, T_SHORT, R->georef.n_geokeys, R->georef.geokeys, (size_t)R->georef.n_geokeys * 2);
    if (R->georef.geodoubles)
        ENT(34736, T_DOUBLE, R->georef.n_geodoubles, R->georef.geodoubles, (size_t)R->georef.n_geodoubles * 8);
    if (R->georef.geoascii)
        ENT(34737, T_ASCII, strlen(R->georef.geoascii) + 1, R->georef.geoascii, strlen(R->georef.geoascii) + 1);
    if (R->metadata || R->metadata_room) {
        /* a COG's reserved room holds at least the empty element, so the directory has the tag either way */
        static const char empty_md[] = "<GDALMetadata>\n</GDALMetadata>\n";
        const char *md = R->metadata ? R->metadata : empty_md;

        ENT(42112, T_ASCII, strlen(md) + 1, md, strlen(md) + 1);
        ents[ne - 1].room = R->metadata_room;
    }
    if (R->nodata >= 0)
        ENT(42113, T_ASCII, strlen(R->nodata_s) + 1, R->nodata_s, strlen(R->nodata_s) + 1);
#undef ENT
    return ne;
}

static size_t ifd_bytes(int ne)
{
    return 2 + (size_t)ne * 12 + 4;
}

/* One IFD: its out-of-line values from *val_pos on (word aligned; *val_pos is advanced past them) and the
 * directory itself at dir_pos, chained to `next`.  fd < 0: sizes only.  0 or -1. */
static int write_ifd(int fd, const struct dirent_w *ents, int ne, uint64_t dir_pos, uint64_t *val_pos, uint32_t next)
{
    const size_t dirbytes = ifd_bytes(ne);
    unsigned char *dir = fd >= 0 ? calloc(1, dirbytes) : NULL;
    uint64_t pos = (*val_pos + 1) & ~1ull;
    int rc = -1;

    if (fd >= 0 && !dir)
        return -1;
    if (dir)
        put16(dir, (unsigned)ne);
    for (int i = 0; i < ne; i++) {
        unsigned char *e = dir ? dir + 2 + i * 12 : NULL;

        if (e) {
            put16(e, ents[i].tag);
            put16(e + 2, ents[i].type);
            put32(e + 4, ents[i].count);
        }
        if (ents[i].nbytes <= 4) {
            if (e)
                memcpy(e + 8, ents[i].data, ents[i].nbytes);
            continue;
        }
        {
            const size_t room = ents[i].room > ents[i].nbytes ? ents[i].room : ents[i].nbytes;

            if (pos + room > 0xffffffffull || (fd >= 0 && write_all(fd, ents[i].data, ents[i].nbytes, pos) != 0))
                goto done;
            if (fd >= 0 && room > ents[i].nbytes) {
                unsigned char *zero = calloc(1, room - ents[i].nbytes);

                if (!zero || write_all(fd, zero, room - ents[i].nbytes, pos + ents[i].nbytes) != 0) {
                    free(zero);
                    goto done;
                }
                free(zero);
            }
            if (e)
                put32(e + 8, (uint32_t)pos);
            pos = (pos + room + 1) & ~1ull;
        }
    }
    if (dir)
        put32(dir + dirbytes - 4, next);
    if (dir_pos + dirbytes > 0xffffffffull || (fd >= 0 && write_all(fd, dir, dirbytes, dir_pos) != 0))
        goto done;
    *val_pos = pos;
    rc = 0;
done:
    free(dir);
    return rc;
}

/* COG: GDAL's ghost area (structural metadata) at offset 8, then every IFD with its values.  Returns the position
 * of the first byte after them; with fd >= 0 the IFDs are written (tile arrays as they are now). */
static const char cog_ghost_body[] = "LAYOUT=IFDS_BEFORE_DATA\nBLOCK_ORDER=ROW_MAJOR\nKNOWN_INCOMPATIBLE_EDITION=NO\n";

static int cog_layout(gcn10_tiff_writer *R, int fd, uint64_t *first, uint64_t *end)
{
    char ghost[128];
    int n = snprintf(ghost, sizeof ghost, "GDAL_STRUCTURAL_METADATA_SIZE=%06d bytes\n%s",
                     (int)(sizeof cog_ghost_body - 1), cog_ghost_body);
    uint64_t pos = (8 + (uint64_t)n + 1) & ~1ull;

    if (fd >= 0 && write_all(fd, ghost, (size_t)n, 8) != 0)
        return -1;
    *first = pos;
    for (int k = 0; k <= R->n_levels; k++) {
        gcn10_tiff_writer *v = k == 0 ? R : R->levels[k - 1];
        struct ifd_vals x;
        struct dirent_w ents[24];
        const int ne = ifd_entries(R, v, &x, ents);
        const uint64_t dir_pos = pos;
        uint64_t val_pos = dir_pos + ifd_bytes(ne);
        uint64_t next;

        /* the next IFD follows this one's values: their end is known from a dry run */
        if (write_ifd(-1, ents, ne, dir_pos, &val_pos, 0) != 0)
            return -1;
        next = k < R->n_levels ? val_pos : 0;
        val_pos = dir_pos + ifd_bytes(ne);
        if (write_ifd(fd, ents, ne, dir_pos, &val_pos, (uint32_t)next) != 0)
            return -1;
        pos = val_pos;
    }
    *end = pos;
    return 0;
}

/* a plain file's one IFD behind the tile data: out-of-line payloads first, then the directory, both word aligned */
static int plain_layout(gcn10_tiff_writer *w, uint64_t *first)
{
    struct ifd_vals x;
    struct dirent_w ents[24];
    const int ne = ifd_entries(w, w, &x, ents);
    uint64_t val_pos = (w->pos + 1) & ~1ull;

    *first = val_pos;
    return write_ifd(-1, ents, ne, 0, first, 0) != 0 || write_ifd(w->fd, ents, ne, *first, &val_pos, 0) != 0 ? -1 : 0;
}

/* every directory of a writer whose tiles are all in, and the header's pointer to the first of them; 0 or -1 (err) */
static int write_directories(gcn10_tiff_writer *w, char *err, size_t errcap)
{
    unsigned char off[4];
    uint64_t first = 0, end = 0;
    bool laid_out;

    if (w->failed)
        goto io_error;
    if (w->direct)
        gcn10_tiff_set_direct(w, false);        /* the directory is not sector sized */
    for (int k = 0; k <= w->n_levels; k++) {
        const gcn10_tiff_writer *v = k == 0 ? w : w->levels[k - 1];
        const size_t nt = (size_t)v->across * (size_t)v->down;

        for (size_t i = 0; i < nt; i++)
            if (v->counts[i] == 0) {
                if (k == 0)
                    snprintf(err, errcap, "write error on %s: tile %zu was never written", w->path, i);
                else
                    snprintf(err, errcap, "write error on %s: tile %zu of overview level %d was never written",
                             w->path, i, k);
                return -1;
            }
    }
    /* a COG's IFDs go into the room create left for them: same entries, same sizes, now with the tile arrays */
    laid_out = w->cog ? cog_layout(w, w->fd, &first, &end) == 0 && end == w->data_start
                      : plain_layout(w, &first) == 0;
    put32(off, (uint32_t)first);
    if (laid_out && write_all(w->fd, off, 4, 4) == 0)
        return 0;
io_error:
    snprintf(err, errcap, "write error on %s", w->path);
    return -1;
}

int gcn10_tiff_finish(gcn10_tiff_writer *w, char *err, size_t errcap)
{
    int rc;

    w = w->root;
    rc = write_directories(w, err, errcap);
    if (w->fd >= 0 && close(w->fd) != 0 && rc == 0) {
        snprintf(err, errcap, "write error closing %s: %s", w->path, strerror(errno));
        rc = -1;
    }
    w->fd = -1;
    if (rc == 0 && rename(w->part, w->path) != 0) {
        snprintf(err, errcap, "write error on %s: %s", w->path, strerror(errno));
        rc = -1;
    }
    if (rc == 0) {
        free(w->part);
        w->part = NULL;             /* nothing left for abort to remove */
    }
    gcn10_tiff_abort(w);
    return rc;
}

/* ------------------------------------------------------------------------ */
/* GDAL tags                                                                 */
/* ------------------------------------------------------------------------ */

/* A COG's directories were laid out at create for the tags set then; a tag that changes their size re-lays them out,
 * which only works before the first tile went behind them.  Called with the root and its lock held. */
static int cog_relayout(gcn10_tiff_writer *R)
{
    uint64_t first, end;

    if (!R->cog)
        return 0;
    if (R->pos != R->data_start || cog_layout(R, -1, &first, &end) != 0)
        return -1;
    R->data_start = end;
    R->pos = end;
    return 0;
}

int gcn10_tiff_set_nodata(gcn10_tiff_writer *w, int v)
{
    int rc = 0, old;

    w = w->root;
    if (v < 0 || v > 255)
        return -1;
    pthread_mutex_lock(&w->mu);
    old = w->nodata;
    w->nodata = v;
    snprintf(w->nodata_s, sizeof w->nodata_s, "%d", v);
    if (old < 0 && cog_relayout(w) != 0) {
        w->nodata = old;
        rc = -1;
    }
    pthread_mutex_unlock(&w->mu);
    return rc;
}

int gcn10_tiff_reserve_metadata(gcn10_tiff_writer *w, size_t bytes)
{
    int rc = 0;
    size_t old;

    w = w->root;
    if (!w->cog)
        return 0;
    if (bytes > 0xffffffu)
        return -1;
    pthread_mutex_lock(&w->mu);
    old = w->metadata_room;
    w->metadata_room = bytes;
    if ((w->metadata && strlen(w->metadata) + 1 > bytes) || cog_relayout(w) != 0) {
        w->metadata_room = old;
        rc = -1;
    }
    pthread_mutex_unlock(&w->mu);
    return rc;
}

int gcn10_tiff_set_metadata_xml(gcn10_tiff_writer *w, const char *xml)
{
    char *copy = NULL;
    int rc = 0;

    w = w->root;
    if (xml && !(copy = strdup(xml)))
        return -1;
    pthread_mutex_lock(&w->mu);
    if (w->cog && copy && strlen(copy) + 1 > w->metadata_room) {
        rc = -1;                    /* a COG's text must fit the room its directory has (reserve_metadata) */
        free(copy);
    }
    else {
        free(w->metadata);
        w->metadata = copy;
    }
    pthread_mutex_unlock(&w->mu);
    return rc;
}

static void free_level_view(gcn10_tiff_writer *v)
{
    if (!v)
        return;
    free(v->offsets);
    free(v->counts);
    free(v);
}

void gcn10_tiff_abort(gcn10_tiff_writer *w)
{
    if (!w)
        return;
    w = w->root ? w->root : w;
    if (w->levels)
        for (int k = 0; k < w->n_levels; k++)
            free_level_view(w->levels[k]);
    free(w->levels);
    if (w->fd >= 0)
        close(w->fd);
    if (w->part)
        unlink(w->part);            /* an unfinished raster is no raster */
    free(w->part);
    free(w->offsets);
    free(w->counts);
    free(w->path);
    free(w->metadata);
    free_georef(&w->georef);
    pthread_mutex_destroy(&w->mu);
    free(w);
}

/* ------------------------------------------------------------------------ */
/* whole rasters from memory                                                 */
/* ------------------------------------------------------------------------ */

size_t gcn10_deflate_tile(const uint8_t *src, size_t stride, int valid_w, int valid_h, int level,
                          uint8_t *dst, size_t dstcap)
{
    unsigned char tile[TILE * TILE];
    uLongf dl = (uLongf)dstcap;

    if (valid_w <= 0 || valid_h <= 0 || valid_w > TILE || valid_h > TILE)
        return 0;
    if (valid_w < TILE || valid_h < TILE)
        memset(tile, 0, sizeof tile);
    for (int y = 0; y < valid_h; y++)
        memcpy(tile + (size_t)y * TILE, src + (size_t)y * stride, (size_t)valid_w);
    if (compress2(dst, &dl, tile, sizeof tile, level > 0 ? level : Z_DEFAULT_COMPRESSION) != Z_OK)
        return 0;
    return (size_t)dl;
}

int gcn10_save_raster(const uint8_t *data, int xsize, int ysize, const double gt[6],
                      const gcn10_georef *georef, const char *path, int level, char *err,
                      size_t errcap)
{
    gcn10_tiff_writer *w = gcn10_tiff_create(path, xsize, ysize, gt, georef, err, errcap);
    size_t cap = compressBound(TILE * TILE);
    uint8_t *z;

    if (!w)
        return -1;
    z = malloc(cap);
    if (!z) {
        snprintf(err, errcap, "out of memory writing %s", path);
        gcn10_tiff_abort(w);
        return -1;
    }
    for (int ty = 0; ty < w->down; ty++) {
        for (int tx = 0; tx < w->across; tx++) {
            int vw = xsize - tx * TILE < TILE ? xsize - tx * TILE : TILE;
            int vh = ysize - ty * TILE < TILE ? ysize - ty * TILE : TILE;
            size_t n = gcn10_deflate_tile(data + (size_t)ty * TILE * (size_t)xsize + (size_t)tx * TILE,
                                          (size_t)xsize, vw, vh, level, z, cap);

            if (n == 0 || gcn10_tiff_put_tile(w, tx, ty, z, n) != 0) {
                snprintf(err, errcap, "write error %d on %s", 3, path);     /* CE_Failure, src/raster.c:221 */
                free(z);
                gcn10_tiff_abort(w);
                return -1;
            }
        }
    }
    free(z);
    return gcn10_tiff_finish(w, err, errcap);
}
