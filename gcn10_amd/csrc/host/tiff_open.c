/* tiff_open.c -- opening one directory of a TIFF / BigTIFF file: header and byte order, the walk along the directory
 * chain, the tags, the chunk layout they imply, the geotransform; and what an open file can be asked about itself.
 * (The module as a whole: tiff_internal.h.)
 */
#include "tiff_internal.h"

#include <errno.h>
#include <fcntl.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

int gcn10_pread_all(int fd, void *buf, size_t n, uint64_t off)
{
    unsigned char *p = buf;

    while (n) {
        ssize_t r = pread(fd, p, n, (off_t)off);

        if (r < 0 && errno == EINTR)
            continue;
        if (r <= 0)
            return -1;
        p += r;
        off += (uint64_t)r;
        n -= (size_t)r;
    }
    return 0;
}

static size_t type_size(unsigned t)
{
    switch (t) {
    case T_BYTE: case T_ASCII: case T_SBYTE: case T_UNDEF: return 1;
    case T_SHORT: case T_SSHORT: return 2;
    case T_LONG: case T_SLONG: case T_FLOAT: case T_IFD: return 4;
    case T_RATIONAL: case T_SRATIONAL: case T_DOUBLE: case T_LONG8: case T_SLONG8: case T_IFD8: return 8;
    default: return 0;
    }
}

/* values of one directory entry as raw bytes (malloc'd), file byte order */
static unsigned char *entry_bytes(struct gcn10_tiff *t, const unsigned char *e, unsigned type,
                                  uint64_t count, size_t *nbytes)
{
    size_t ts = type_size(type);
    size_t inl = t->big ? 8 : 4;
    const unsigned char *valp = e + (t->big ? 12 : 8);
    unsigned char *buf;

    /* a value array can never be larger than the file that holds it */
    if (!ts || count > (1ull << 31) / ts || ts * count > t->file_size)
        return NULL;
    *nbytes = (size_t)(ts * count);
    buf = malloc(*nbytes ? *nbytes : 1);
    if (!buf)
        return NULL;
    if (*nbytes <= inl) {
        memcpy(buf, valp, *nbytes);
    }
    else {
        uint64_t off = rd(valp, (int)inl, t->swap);

        if (gcn10_pread_all(t->fd, buf, *nbytes, off) != 0) {
            free(buf);
            return NULL;
        }
    }
    return buf;
}

static uint64_t *entry_u64(struct gcn10_tiff *t, const unsigned char *e, unsigned type, uint64_t count)
{
    size_t nb = 0, ts = type_size(type);
    unsigned char *raw = entry_bytes(t, e, type, count, &nb);
    uint64_t *out;

    if (!raw)
        return NULL;
    out = malloc((size_t)(count ? count : 1) * sizeof *out);
    if (out)
        for (uint64_t i = 0; i < count; i++)
            out[i] = rd(raw + i * ts, (int)ts, t->swap);
    free(raw);
    return out;
}

static double *entry_f64(struct gcn10_tiff *t, const unsigned char *e, unsigned type, uint64_t count)
{
    uint64_t *bits = type == T_DOUBLE ? entry_u64(t, e, type, count) : NULL;
    double *out = bits ? malloc((size_t)(count ? count : 1) * sizeof *out) : NULL;

    if (out)
        memcpy(out, bits, (size_t)count * sizeof *out);
    free(bits);
    return out;
}

void gcn10_tiff_close_reader(struct gcn10_tiff *t)
{
    if (!t)
        return;
    if (t->fd >= 0)
        close(t->fd);
    free(t->offsets);
    free(t->counts);
    free(t->georef.geokeys);
    free(t->georef.geodoubles);
    free(t->georef.geoascii);
    free(t);
}

struct gcn10_tiff *gcn10_tiff_open_reader(const char *path, char *err, size_t errcap)
{
    return gcn10_tiff_open_reader_ifd(path, 0, NULL, err, errcap);
}

/* Where an open's refusal goes.  A step of the open answers 0, BAD (the file's structure: the caller writes the one
 * message for that) or REFUSED (the step has said why itself). */
struct report {
    const char *path;
    int *why;
    char *err;
    size_t errcap;
};
enum { BAD = 1, REFUSED = 2 };

/* "gdal open failed: <path><what>" (src/raster.c:121), *why = code unless 0; returns REFUSED */
static int refuse(const struct report *r, int code, const char *what, ...)
{
    char tail[160];
    va_list ap;

    va_start(ap, what);
    vsnprintf(tail, sizeof tail, what, ap);
    va_end(ap);
    if (r->why && code)
        *r->why = code;
    snprintf(r->err, r->errcap, "gdal open failed: %s%s", r->path, tail);
    return REFUSED;
}

/* what the directory's entries say that is not a field of the open file itself, before any of it is checked */
struct raw_tags {
    uint32_t rows_per_strip, tile_w, tile_h;
    bool have_off, have_cnt;
    double *scale, *tie, *xform;
    uint64_t n_scale, n_tie, n_xform;
};

/* step 1: the file, its size and identity, byte order, classic or BigTIFF; *ifd = where the first directory lies */
static int read_header(struct gcn10_tiff *t, const struct report *r, uint64_t *ifd)
{
    unsigned char hdr[16];
    struct stat st;
    unsigned magic;

    t->fd = open(r->path, O_RDONLY);
    if (t->fd < 0 || gcn10_pread_all(t->fd, hdr, 8, 0) != 0)
        return refuse(r, t->fd < 0 && errno == ENOENT ? GCN10_TIFF_E_MISSING : 0, "");
    if (fstat(t->fd, &st) != 0 || st.st_size < 8)
        return BAD;
    t->file_size = (uint64_t)st.st_size;
    t->id_dev = (uint64_t)st.st_dev;
    t->id_ino = (uint64_t)st.st_ino;
    if (hdr[0] == 'I' && hdr[1] == 'I')
        t->swap = false;
    else if (hdr[0] == 'M' && hdr[1] == 'M')
        t->swap = true;
    else
        return refuse(r, 0, " (not a TIFF)");
    magic = (unsigned)rd(hdr + 2, 2, t->swap);
    if (magic == 42) {
        *ifd = rd(hdr + 4, 4, t->swap);
        return 0;
    }
    if (magic != 43 || gcn10_pread_all(t->fd, hdr, 16, 0) != 0)
        return BAD;
    t->big = true;
    *ifd = rd(hdr + 8, 8, t->swap);
    return 0;
}

/* step 2: along the chain to directory `level`; its entries (malloc'd) and their number */
static int walk_to_directory(struct gcn10_tiff *t, const struct report *r, int level, uint64_t ifd,
                             unsigned char **dir, uint64_t *nent)
{
    const int cn = t->big ? 8 : 2, on = t->big ? 8 : 4;
    const size_t esz = t->big ? 20 : 12;

    for (int k = 0;; k++) {
        unsigned char cnt[8], next[8];

        if (gcn10_pread_all(t->fd, cnt, (size_t)cn, ifd) != 0)
            return BAD;
        *nent = rd(cnt, cn, t->swap);
        if (*nent == 0 || *nent > 4096)
            return BAD;
        /* the chain's next directory (0: this is the last one); a file that ends right behind its entries has none */
        t->next_ifd = gcn10_pread_all(t->fd, next, (size_t)on, ifd + (uint64_t)cn + *nent * esz) == 0
                          ? rd(next, on, t->swap) : 0;
        if (k >= level)
            break;
        if (t->next_ifd == 0 || k >= 64)
            return refuse(r, GCN10_TIFF_E_NO_IFD, " has no directory %d", level);
        ifd = t->next_ifd;
    }
    *dir = malloc((size_t)*nent * esz);
    if (!*dir || gcn10_pread_all(t->fd, *dir, (size_t)*nent * esz, ifd + (uint64_t)cn) != 0)
        return BAD;
    return 0;
}

/* step 3: the entries' values, into t and *tags; BAD only for a scalar tag without a readable value */
static int read_tags(struct gcn10_tiff *t, const unsigned char *dir, uint64_t nent, struct raw_tags *tags)
{
    const size_t esz = t->big ? 20 : 12;

    t->bps = 1;
    t->spp = 1;
    t->compression = 1;
    t->predictor = 1;
    t->planar = 1;
    for (uint64_t i = 0; i < nent; i++) {
        const unsigned char *e = dir + i * esz;
        unsigned tag = (unsigned)rd(e, 2, t->swap);
        unsigned type = (unsigned)rd(e + 2, 2, t->swap);
        uint64_t count = t->big ? rd(e + 4, 8, t->swap) : rd(e + 4, 4, t->swap);
        uint64_t *v = NULL;

        switch (tag) {
        case 256: case 257: case 258: case 259: case 277: case 278: case 284: case 317:
        case 322: case 323:
            v = entry_u64(t, e, type, count);
            if (!v || count < 1) {
                free(v);
                return BAD;
            }
            if (tag == 256) t->width = (uint32_t)v[0];
            else if (tag == 257) t->height = (uint32_t)v[0];
            else if (tag == 258) t->bps = (uint16_t)v[0];
            else if (tag == 259) t->compression = (uint16_t)v[0];
            else if (tag == 277) t->spp = (uint16_t)v[0];
            else if (tag == 278) tags->rows_per_strip = (uint32_t)v[0];
            else if (tag == 284) t->planar = (uint16_t)v[0];
            else if (tag == 317) t->predictor = (uint16_t)v[0];
            else if (tag == 322) tags->tile_w = (uint32_t)v[0];
            else if (tag == 323) tags->tile_h = (uint32_t)v[0];
            free(v);
            break;
        case 273: case 324:         /* StripOffsets / TileOffsets */
            free(t->offsets);
            t->offsets = entry_u64(t, e, type, count);
            t->n_chunks = count;
            tags->have_off = t->offsets != NULL;
            if (tag == 324)
                t->tiled = true;
            break;
        case 279: case 325:         /* StripByteCounts / TileByteCounts */
            free(t->counts);
            t->counts = entry_u64(t, e, type, count);
            tags->have_cnt = t->counts != NULL;
            break;
        case 33550:
            free(tags->scale);
            tags->scale = entry_f64(t, e, type, count);
            tags->n_scale = count;
            break;
        case 33922:
            free(tags->tie);
            tags->tie = entry_f64(t, e, type, count);
            tags->n_tie = count;
            break;
        case 34264:
            free(tags->xform);
            tags->xform = entry_f64(t, e, type, count);
            tags->n_xform = count;
            break;
        case 34735:
            v = entry_u64(t, e, type, count);
            if (v) {
                free(t->georef.geokeys);
                t->georef.geokeys = malloc((size_t)(count ? count : 1) * sizeof(uint16_t));
                if (t->georef.geokeys) {
                    for (uint64_t k = 0; k < count; k++)
                        t->georef.geokeys[k] = (uint16_t)v[k];
                    t->georef.n_geokeys = (int)count;
                }
                free(v);
            }
            break;
        case 34736:
            free(t->georef.geodoubles);
            t->georef.geodoubles = entry_f64(t, e, type, count);
            t->georef.n_geodoubles = t->georef.geodoubles ? (int)count : 0;
            break;
        case 34737: {
            size_t nb = 0;
            unsigned char *raw = entry_bytes(t, e, T_ASCII, count, &nb);

            if (raw) {
                free(t->georef.geoascii);
                t->georef.geoascii = malloc(nb + 1);
                if (t->georef.geoascii) {
                    memcpy(t->georef.geoascii, raw, nb);
                    t->georef.geoascii[nb] = '\0';
                }
                free(raw);
            }
            break;
        }
        default:
            break;
        }
    }
    return 0;
}

/* step 4: what the tags must say for this reader, and the chunk grid they imply */
static int derive_layout(struct gcn10_tiff *t, const struct report *r, const struct raw_tags *tags)
{
    if (!t->width || !t->height || !tags->have_off || !tags->have_cnt)
        return BAD;
    t->spp_file = t->spp;
    if (t->bps != 8)
        return refuse(r, GCN10_TIFF_E_NOT_BYTE, " (%u bits per sample; only Byte rasters are supported)", t->bps);
    if (t->planar != 1 && t->spp != 1) {
        /* band-sequential: band 1 is the first n_chunks / spp chunks */
        t->n_chunks /= t->spp;
        t->spp = 1;
    }
    if (t->tiled) {
        if (!tags->tile_w || !tags->tile_h)
            return BAD;
        t->cw = tags->tile_w;
        t->ch = tags->tile_h;
    }
    else {
        t->cw = t->width;
        t->ch = tags->rows_per_strip && tags->rows_per_strip < t->height ? tags->rows_per_strip : t->height;
    }
    t->across = (t->width + t->cw - 1) / t->cw;
    t->down = (t->height + t->ch - 1) / t->ch;
    if ((uint64_t)t->across * t->down > t->n_chunks)
        return BAD;
    if (t->spp == 0 || t->spp > 16 || (uint64_t)t->cw * t->ch * t->spp > (1ull << 30) ||
        t->width > 0x7fffffffu || t->height > 0x7fffffffu)
        return BAD;
    switch (t->compression) {
    case 1: case 5: case 8: case 32946: case 32773:
        return 0;
    default:
        return refuse(r, 0, " (TIFF compression %u not supported)", t->compression);
    }
}

/* step 5: the geotransform in GDAL order {x0, dx, rx, y0, ry, dy} */
static void derive_geotransform(struct gcn10_tiff *t, const struct raw_tags *tags)
{
    const double *xform = tags->xform, *scale = tags->scale, *tie = tags->tie;

    t->gt[0] = 0; t->gt[1] = 1; t->gt[2] = 0; t->gt[3] = 0; t->gt[4] = 0; t->gt[5] = 1;
    if (xform && tags->n_xform >= 16) {
        t->gt[0] = xform[3]; t->gt[1] = xform[0]; t->gt[2] = xform[1];
        t->gt[3] = xform[7]; t->gt[4] = xform[4]; t->gt[5] = xform[5];
    }
    else if (scale && tags->n_scale >= 2 && tie && tags->n_tie >= 6) {
        /* GDAL: origin = tiepoint world - tiepoint pixel * scale; north-up */
        t->gt[1] = scale[0];
        t->gt[5] = -scale[1];
        t->gt[0] = tie[3] - tie[0] * scale[0];
        t->gt[3] = tie[4] + tie[1] * scale[1];
    }
    /* RasterPixelIsPoint (GTRasterTypeGeoKey 1025 = 2) shifts by half a pixel, as GDAL does */
    if (t->georef.geokeys && t->georef.n_geokeys >= 4) {
        int nk = t->georef.geokeys[3];

        for (int k = 0; k < nk && 4 + 4 * k + 3 < t->georef.n_geokeys; k++) {
            const uint16_t *key = t->georef.geokeys + 4 + 4 * k;

            if (key[0] == 1025 && key[1] == 0 && key[3] == 2) {
                t->gt[0] -= 0.5 * t->gt[1] + 0.5 * t->gt[2];
                t->gt[3] -= 0.5 * t->gt[4] + 0.5 * t->gt[5];
            }
        }
    }
}

/* directory `level` of the file's chain (0 = the first: the raster itself; k = the k-th one behind it: overview k
 * of a Cloud Optimized GeoTIFF).  *why (optional) says what kind of failure a NULL is: GCN10_TIFF_E_* */
struct gcn10_tiff *gcn10_tiff_open_reader_ifd(const char *path, int level, int *why, char *err, size_t errcap)
{
    const struct report r = { path, why, err, errcap };
    struct gcn10_tiff *t = calloc(1, sizeof *t);
    struct raw_tags tags = { 0 };
    unsigned char *dir = NULL;
    uint64_t ifd = 0, nent = 0;
    int rc;

    if (!t) {
        snprintf(err, errcap, "out of memory for raster %s", path);
        return NULL;
    }
    if (why)
        *why = GCN10_TIFF_E_STRUCTURE;
    rc = read_header(t, &r, &ifd);
    if (rc == 0)
        rc = walk_to_directory(t, &r, level, ifd, &dir, &nent);
    if (rc == 0)
        rc = read_tags(t, dir, nent, &tags);
    if (rc == 0)
        rc = derive_layout(t, &r, &tags);
    if (rc == 0)
        derive_geotransform(t, &tags);
    free(dir);
    free(tags.scale);
    free(tags.tie);
    free(tags.xform);
    if (rc == 0)
        return t;
    if (rc == BAD)
        refuse(&r, 0, " (unreadable or unsupported TIFF structure)");
    gcn10_tiff_close_reader(t);
    return NULL;
}

void gcn10_tiff_reader_info(const struct gcn10_tiff *t, int *xsize, int *ysize, double gt[6])
{
    *xsize = (int)t->width;
    *ysize = (int)t->height;
    memcpy(gt, t->gt, sizeof t->gt);
}

const gcn10_georef *gcn10_tiff_reader_georef(const struct gcn10_tiff *t)
{
    return &t->georef;
}

int gcn10_tiff_reader_samples(const struct gcn10_tiff *t)
{
    return t->spp_file;
}

bool gcn10_tiff_reader_has_next(const struct gcn10_tiff *t)
{
    return t->next_ifd != 0;
}

bool gcn10_tiff_chunk_in_file(const struct gcn10_tiff *t, uint64_t idx)
{
    return t->offsets[idx] <= t->file_size && t->counts[idx] <= t->file_size - t->offsets[idx];
}

/* The first chunk of the raster that cannot hold pixels: no bytes at all (a sparse chunk, which reads as zeros), or
 * bytes that reach beyond the end of the file.  0 = every chunk is in the file; 1 = *index / *off / *count name one. */
int gcn10_tiff_check_chunks(const struct gcn10_tiff *t, uint64_t *index, uint64_t *off, uint64_t *count)
{
    for (uint64_t i = 0; i < (uint64_t)t->across * t->down; i++) {
        if (t->counts[i] != 0 && gcn10_tiff_chunk_in_file(t, i))
            continue;
        *index = i;
        *off = t->offsets[i];
        *count = t->counts[i];
        return 1;
    }
    return 0;
}
