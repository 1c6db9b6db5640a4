/* zones.c -- the polygon shapefile of zones and its scan conversion over a block (config key "zonal").
 *
 * gcn10_blocks_open (blocks.c) needs a record's bounding box only; zones need the rings.  The reader takes foreign
 * files, so nothing of a file is used before it has been checked against the file's size.  The scan conversion is a
 * scanline with an active-edge list: the edges of a zone are put into the bucket of the first row they cross, a row
 * evaluates the edges active in it, and an edge leaves after its last row -- O(edges + rows touched + crossings) per
 * zone, not rows x edges (a zone can have 1e5 vertices and a block has 36001 rows).
 *
 * The membership rule is stated in include/gcn10_host.h and is evaluated here exactly as stated, in plain IEEE double
 * (this file is built with -ffp-contract=off): which rows an edge crosses and which columns lie right of a crossing
 * are found from an estimate that is then corrected with the rule's own comparisons, so the estimate's rounding
 * never decides a pixel.
 */
#include "gcn10_host.h"
#include "bytes.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>

#if defined(__GNUC__) && !defined(__clang__)
#define NO_CONTRACT __attribute__((optimize("fp-contract=off")))
#else
#define NO_CONTRACT
#pragma STDC FP_CONTRACT OFF
#endif

/* Bounds of a span and of an item, in pixels.  Results never depend on them.  Chosen from the sweep of
 * tools/bench_zonal.py (profiles/zonal/kernel_bounds.json, one zone over a 36000 x 2304 strip, against 0.049 ms of
 * gcn10_gpu_pair_histogram on the same strip):
 *   span:item      1024:16384  4096:16384  4096:65536  16384:65536  4096:262144  36000:288000
 *   ms (patchy)    0.076       0.072       0.080       0.068        0.132        0.129
 * Longer spans mean fewer of them to lay out and search (6 912 instead of 20 736); items must outnumber the 1 024
 * workgroups of a launch (320 and 288 items leave most of the device idle), and 1 536 items of 65536 px do. */
enum { DEFAULT_SPAN_PX = 16384, DEFAULT_ITEM_PX = 65536 };

/* ---------------------------------------------------------------------------------------------------------------- */
/* reader                                                                                                            */
/* ---------------------------------------------------------------------------------------------------------------- */

static unsigned char *slurp(const char *path, size_t *len)
{
    FILE *f = fopen(path, "rb");
    unsigned char *buf;
    long n;

    if (!f)
        return NULL;
    if (fseek(f, 0, SEEK_END) != 0 || (n = ftell(f)) < 0 || fseek(f, 0, SEEK_SET) != 0) {
        fclose(f);
        return NULL;
    }
    buf = malloc((size_t)n + 1);
    if (!buf || fread(buf, 1, (size_t)n, f) != (size_t)n) {
        free(buf);
        fclose(f);
        return NULL;
    }
    fclose(f);
    *len = (size_t)n;
    return buf;
}

/* "<base>.shp" -> "<base>.dbf" (keeps the case of the extension) */
static char *dbf_path_of(const char *shp_path)
{
    size_t n = strlen(shp_path);
    char *out = malloc(n + 5);

    if (!out)
        return NULL;
    memcpy(out, shp_path, n + 1);
    if (n >= 4 && out[n - 4] == '.')
        memcpy(out + n - 3, out[n - 1] >= 'A' && out[n - 1] <= 'Z' ? "DBF" : "dbf", 3);
    else
        memcpy(out + n, ".dbf", 5);
    return out;
}

/* the numeric column `field` of the first n records, record i of the .dbf belonging to record i of the .shp */
static int read_dbf_ids(const char *path, const char *field, int n, int64_t *ids, char *err, size_t errcap)
{
    size_t len = 0;
    unsigned char *d = slurp(path, &len);
    size_t hdr, rec, fld_off = 1, fld_len = 0;
    uint32_t nrec;
    bool found = false;

    if (!d || len < 32) {
        snprintf(err, errcap, "cannot read %s", path);
        free(d);
        return -1;
    }
    nrec = le32(d + 4);
    hdr = (size_t)d[8] | ((size_t)d[9] << 8);
    rec = (size_t)d[10] | ((size_t)d[11] << 8);
    for (size_t p = 32; p + 32 <= hdr && p + 32 <= len && d[p] != 0x0D; p += 32) {
        char name[12];

        memcpy(name, d + p, 11);
        name[11] = '\0';
        if (strcasecmp(name, field) == 0) {
            if (d[p + 11] != 'N' && d[p + 11] != 'F') {
                snprintf(err, errcap, "%s: field \"%s\" is not numeric", path, field);
                free(d);
                return -1;
            }
            fld_len = d[p + 16];
            found = true;
            break;
        }
        fld_off += d[p + 16];
    }
    if (!found) {
        snprintf(err, errcap, "%s has no \"%s\" field", path, field);
        free(d);
        return -1;
    }
    if (hdr < 33 || rec < 1 || fld_off + fld_len > rec) {
        snprintf(err, errcap, "%s: field \"%s\" lies outside the records", path, field);
        free(d);
        return -1;
    }
    if ((uint64_t)nrec < (uint64_t)n || (uint64_t)hdr + (uint64_t)n * rec > (uint64_t)len) {
        snprintf(err, errcap, "%s has fewer than the %d records of the .shp", path, n);
        free(d);
        return -1;
    }
    for (int i = 0; i < n; i++) {
        char tmp[64];
        const size_t m = fld_len < 63 ? fld_len : 63;

        memcpy(tmp, d + hdr + (size_t)i * rec + fld_off, m);
        tmp[m] = '\0';
        ids[i] = (int64_t)strtoll(tmp, NULL, 10);
    }
    free(d);
    return 0;
}

void gcn10_zones_free(gcn10_zones *z)
{
    free(z->id);
    free(z->bbox);
    free(z->ring_first);
    free(z->ring_pt);
    free(z->xy);
    memset(z, 0, sizeof *z);
}

int gcn10_zones_open(const char *shp_path, const char *id_field, gcn10_zones *out, char *err, size_t errcap)
{
    size_t len = 0, pos;
    unsigned char *s = slurp(shp_path, &len);
    uint64_t n_rec = 0, n_rings = 0, n_points = 0, ri = 0, pi = 0;
    char *dbf = NULL;
    int rc = -1;

    memset(out, 0, sizeof *out);
    if (!s || len < 100 || be32(s) != 9994) {
        snprintf(err, errcap, "cannot read the zones of %s: not a shapefile", shp_path);
        free(s);
        return -1;
    }
    /* pass 1: every record checked against the file, and the sizes of the arrays */
    for (pos = 100; pos < len; n_rec++) {
        uint64_t content;
        const unsigned char *rec;
        uint32_t type;

        if (len - pos < 8) {
            snprintf(err, errcap, "%s: record %llu: header beyond the end of the file", shp_path,
                     (unsigned long long)n_rec + 1);
            goto out;
        }
        content = (uint64_t)be32(s + pos + 4) * 2;          /* 16-bit words */
        rec = s + pos + 8;
        if (content > len - pos - 8 || content < 4) {
            snprintf(err, errcap, "%s: record %llu: length %llu beyond the end of the file", shp_path,
                     (unsigned long long)n_rec + 1, (unsigned long long)content);
            goto out;
        }
        type = le32(rec);
        if (type == 5 || type == 15 || type == 25) {
            uint64_t np, npt;

            if (content < 44) {
                snprintf(err, errcap, "%s: record %llu: too short for a polygon", shp_path, (unsigned long long)n_rec + 1);
                goto out;
            }
            np = le32(rec + 36);
            npt = le32(rec + 40);
            if (44 + 4 * np + 16 * npt > content || (npt > 0 && np == 0)) {
                snprintf(err, errcap, "%s: record %llu: %llu parts and %llu points do not fit its %llu bytes", shp_path,
                         (unsigned long long)n_rec + 1, (unsigned long long)np, (unsigned long long)npt,
                         (unsigned long long)content);
                goto out;
            }
            for (uint64_t k = 0; k < np; k++) {
                const uint32_t at = le32(rec + 44 + 4 * k);

                if ((k == 0 ? at != 0 : at < le32(rec + 44 + 4 * (k - 1))) || (at >= npt && !(npt == 0 && at == 0))) {
                    snprintf(err, errcap, "%s: record %llu: part %llu starts at point %u of %llu (parts must start at 0, "
                             "ascend and lie inside the points)", shp_path, (unsigned long long)n_rec + 1,
                             (unsigned long long)k, at, (unsigned long long)npt);
                    goto out;
                }
            }
            n_rings += np;
            n_points += npt;
        }
        else if (type != 0) {
            snprintf(err, errcap, "%s: record %llu: shape type %u is not a polygon (5, 15, 25) or a null shape", shp_path,
                     (unsigned long long)n_rec + 1, type);
            goto out;
        }
        pos += 8 + (size_t)content;
    }
    if (n_rec > 0x7fffffffu) {
        snprintf(err, errcap, "%s: too many records", shp_path);
        goto out;
    }
    out->n = (int)n_rec;
    out->n_rings = n_rings;
    out->n_points = n_points;
    out->id = calloc((size_t)n_rec + 1, sizeof *out->id);
    out->bbox = calloc((size_t)n_rec + 1, sizeof *out->bbox);
    out->ring_first = calloc((size_t)n_rec + 1, sizeof *out->ring_first);
    out->ring_pt = calloc((size_t)n_rings + 1, sizeof *out->ring_pt);
    out->xy = calloc((size_t)n_points + 1, 2 * sizeof *out->xy);
    if (!out->id || !out->bbox || !out->ring_first || !out->ring_pt || !out->xy) {
        snprintf(err, errcap, "%s: out of memory for %llu points", shp_path, (unsigned long long)n_points);
        goto out;
    }
    /* pass 2: the same walk, filling them */
    pos = 100;
    for (uint64_t i = 0; i < n_rec; i++) {
        const uint64_t content = (uint64_t)be32(s + pos + 4) * 2;
        const unsigned char *rec = s + pos + 8;
        const uint32_t type = le32(rec);

        out->ring_first[i] = ri;
        if (type != 0) {
            const uint64_t np = le32(rec + 36), npt = le32(rec + 40);
            const unsigned char *pts = rec + 44 + 4 * np;

            /* the box of the points themselves: the one in the record header is not believed, since the rows scanned
             * for a zone come from it and a wrong one would lose pixels silently */
            for (uint64_t k = 0; k < np; k++)
                out->ring_pt[ri++] = pi + le32(rec + 44 + 4 * k);
            for (uint64_t k = 0; k < npt; k++, pi++) {
                const double x = le_f64(pts + 16 * k), y = le_f64(pts + 16 * k + 8);

                if (!isfinite(x) || !isfinite(y)) {
                    snprintf(err, errcap, "%s: record %llu: point %llu is not finite", shp_path, (unsigned long long)i + 1,
                             (unsigned long long)k);
                    goto out;
                }
                out->xy[2 * pi] = x;
                out->xy[2 * pi + 1] = y;
                if (k == 0 || x < out->bbox[i][0])
                    out->bbox[i][0] = x;
                if (k == 0 || y < out->bbox[i][1])
                    out->bbox[i][1] = y;
                if (k == 0 || x > out->bbox[i][2])
                    out->bbox[i][2] = x;
                if (k == 0 || y > out->bbox[i][3])
                    out->bbox[i][3] = y;
            }
        }
        pos += 8 + (size_t)content;
    }
    out->ring_first[n_rec] = ri;
    out->ring_pt[n_rings] = pi;

    dbf = dbf_path_of(shp_path);
    if (!dbf) {
        snprintf(err, errcap, "%s: out of memory", shp_path);
        goto out;
    }
    rc = read_dbf_ids(dbf, id_field && *id_field ? id_field : "ID", out->n, out->id, err, errcap);
out:
    free(dbf);
    free(s);
    if (rc != 0)
        gcn10_zones_free(out);
    return rc;
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* items                                                                                                             */
/* ---------------------------------------------------------------------------------------------------------------- */

struct span_list {
    gcn10_zone_span *v;
    size_t n, cap;
};

static int span_push(struct span_list *l, int32_t y, int32_t x0, int32_t x1, int32_t zone, uint32_t max_span_px)
{
    while (x0 < x1) {
        const int32_t end = (uint32_t)(x1 - x0) > max_span_px ? x0 + (int32_t)max_span_px : x1;

        if (l->n == l->cap) {
            const size_t cap = l->cap ? l->cap * 2 : 1024;
            gcn10_zone_span *g = realloc(l->v, cap * sizeof *g);

            if (!g)
                return -1;
            l->v = g;
            l->cap = cap;
        }
        l->v[l->n++] = (gcn10_zone_span){ y, x0, end, zone };
        x0 = end;
    }
    return 0;
}

static void bounds_of(uint32_t *max_span_px, uint32_t *max_item_px)
{
    if (*max_span_px == 0)
        *max_span_px = DEFAULT_SPAN_PX;
    if (*max_item_px == 0)
        *max_item_px = DEFAULT_ITEM_PX;
    if (*max_span_px > 0x40000000u)
        *max_span_px = 0x40000000u;
    if (*max_item_px < *max_span_px)
        *max_item_px = *max_span_px;
}

/* items over spans sorted by zone: consecutive spans of one zone, at most max_item_px pixels each */
static int items_of(const gcn10_zone_span *sp, size_t n, uint32_t max_item_px, gcn10_zone_item **items, size_t *n_items)
{
    size_t cap = 256, m = 0;
    gcn10_zone_item *it = malloc(cap * sizeof *it);

    *items = NULL;
    *n_items = 0;
    if (!it || n > 0xffffffffu) {
        free(it);
        return -1;
    }
    for (size_t i = 0; i < n;) {
        uint64_t px = 0;
        size_t j = i;

        while (j < n && sp[j].zone == sp[i].zone && (j == i || px + (uint64_t)(sp[j].x1 - sp[j].x0) <= max_item_px)) {
            px += (uint64_t)(sp[j].x1 - sp[j].x0);
            j++;
        }
        if (m == cap) {
            gcn10_zone_item *g = realloc(it, cap * 2 * sizeof *g);

            if (!g) {
                free(it);
                return -1;
            }
            it = g;
            cap *= 2;
        }
        it[m++] = (gcn10_zone_item){ (uint32_t)i, (uint32_t)(j - i) };
        i = j;
    }
    *items = it;
    *n_items = m;
    return 0;
}

void gcn10_zone_plan_free(gcn10_zone_plan *p)
{
    free(p->local_zone);
    free(p->local_pixels);
    free(p->spans);
    free(p->items);
    memset(p, 0, sizeof *p);
}

int gcn10_zone_items_build(const gcn10_zone_span *spans, size_t n_spans, uint32_t max_span_px, uint32_t max_item_px,
                           gcn10_zone_plan *out)
{
    struct span_list l = { NULL, 0, 0 };

    memset(out, 0, sizeof *out);
    bounds_of(&max_span_px, &max_item_px);
    for (size_t i = 0; i < n_spans; i++)
        if (spans[i].x0 >= spans[i].x1 || span_push(&l, spans[i].y, spans[i].x0, spans[i].x1, spans[i].zone, max_span_px) != 0) {
            free(l.v);
            return -1;
        }
    if (items_of(l.v, l.n, max_item_px, &out->items, &out->n_items) != 0) {
        free(l.v);
        return -1;
    }
    out->spans = l.v;
    out->n_spans = l.n;
    return 0;
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* scan conversion                                                                                                   */
/* ---------------------------------------------------------------------------------------------------------------- */

enum { GE = 0, GT = 1, LT = 2, LE = 3 };

NO_CONTRACT static inline double centre(double a, double b, int i)
{
    return a + (i + 0.5) * b;
}

static inline bool holds(double c, double v, int mode)
{
    return mode == GE ? c >= v : (mode == GT ? c > v : (mode == LT ? c < v : c <= v));
}

/* The smallest i in [lo, hi] whose centre a + (i + 0.5) * b stands in relation `mode` to v (hi: none below it does).
 * The relation must be false, then true, as i grows: GE and GT with b > 0 (columns), LT and LE with b < 0 (rows).
 * The division only gives the place to start; the centres' own comparisons decide. */
NO_CONTRACT static int first_index(double a, double b, int lo, int hi, double v, int mode)
{
    const double est = ceil((v - a) / b - 0.5);
    int i;

    if (!(v == v))
        return hi;
    i = !(est > (double)lo) ? lo : (est >= (double)hi ? hi : (int)est);
    while (i > lo && holds(centre(a, b, i - 1), v, mode))
        i--;
    while (i < hi && !holds(centre(a, b, i), v, mode))
        i++;
    return i;
}

struct edge {
    double xl, yl, xh, yh;  /* from the endpoint of smaller y (xl, yl) to the other */
    int last;               /* last row it crosses */
    int next;               /* chain of the bucket of its first row */
};

static int by_double(const void *a, const void *b)
{
    const double x = *(const double *)a, y = *(const double *)b;

    return x < y ? -1 : (x > y ? 1 : 0);
}

struct scratch {
    struct edge *edges;
    size_t edges_cap;
    int *head;              /* first edge of each row's bucket */
    size_t head_cap;
    int *active;
    size_t active_cap;
    double *cross;
    size_t cross_cap;
};

static int grow(void **p, size_t *cap, size_t need, size_t elem)
{
    void *g;

    if (need <= *cap)
        return 0;
    need += need / 2 + 64;
    g = realloc(*p, need * elem);
    if (!g)
        return -1;
    *p = g;
    *cap = need;
    return 0;
}

/* spans of one zone (record zi) inside rows [ry0, ry1] and columns [cx0, cx1) of the block; -1 = out of memory */
NO_CONTRACT static int scan_zone(const gcn10_zones *z, int zi, const double gt[6], int W, int ry0, int ry1, int cx0, int cx1,
                                 int32_t local, uint32_t max_span_px, struct scratch *sc, struct span_list *out)
{
    const uint64_t r0 = z->ring_first[zi], r1 = z->ring_first[zi + 1];
    const int nrows = ry1 - ry0 + 1;
    size_t n_edges = 0, n_active = 0;

    if (r1 > r0 && grow((void **)&sc->edges, &sc->edges_cap, (size_t)(z->ring_pt[r1] - z->ring_pt[r0]) + (size_t)(r1 - r0),
                        sizeof *sc->edges) != 0)
        return -1;
    if (grow((void **)&sc->head, &sc->head_cap, (size_t)nrows, sizeof *sc->head) != 0)
        return -1;
    for (int i = 0; i < nrows; i++)
        sc->head[i] = -1;

    /* the edges that cross a row of the range, each into the bucket of its first row */
    for (uint64_t k = r0; k < r1; k++) {
        const uint64_t p0 = z->ring_pt[k], p1 = z->ring_pt[k + 1];

        for (uint64_t p = p0; p < p1; p++) {
            const uint64_t q = p + 1 < p1 ? p + 1 : p0;     /* the last point connects to the first: an open ring is closed */
            const double x1 = z->xy[2 * p], y1 = z->xy[2 * p + 1], x2 = z->xy[2 * q], y2 = z->xy[2 * q + 1];
            const double ylo = y1 < y2 ? y1 : y2, yhi = y1 < y2 ? y2 : y1;
            int first, last;

            if (y1 == y2)
                continue;
            /* (y1 <= py) != (y2 <= py)  <=>  ylo <= py < yhi; py falls as the row grows */
            first = first_index(gt[3], gt[5], ry0, ry1 + 1, yhi, LT);
            if (first > ry1)
                continue;
            last = first_index(gt[3], gt[5], ry0, ry1 + 1, ylo, LT) - 1;
            if (last < first)
                continue;
            /* stored from the lower endpoint, so that both rings of a shared edge evaluate the same crossing */
            sc->edges[n_edges] = y1 < y2 ? (struct edge){ x1, y1, x2, y2, last, sc->head[first - ry0] }
                                         : (struct edge){ x2, y2, x1, y1, last, sc->head[first - ry0] };
            sc->head[first - ry0] = (int)n_edges++;
        }
    }
    if (n_edges == 0)
        return 0;
    if (grow((void **)&sc->active, &sc->active_cap, n_edges, sizeof *sc->active) != 0)
        return -1;
    if (grow((void **)&sc->cross, &sc->cross_cap, n_edges, sizeof *sc->cross) != 0)
        return -1;

    for (int y = ry0; y <= ry1; y++) {
        const double py = centre(gt[3], gt[5], y);
        size_t n = 0;

        for (int e = sc->head[y - ry0]; e >= 0; e = sc->edges[e].next)
            sc->active[n_active++] = e;
        if (n_active == 0)
            continue;
        for (size_t a = 0; a < n_active;) {
            const struct edge *e = &sc->edges[sc->active[a]];

            sc->cross[n++] = e->xl + (py - e->yl) * (e->xh - e->xl) / (e->yh - e->yl);
            if (e->last <= y)
                sc->active[a] = sc->active[--n_active];
            else
                a++;
        }
        if (n > 16)
            qsort(sc->cross, n, sizeof *sc->cross, by_double);
        else
            for (size_t i = 1; i < n; i++) {
                const double c = sc->cross[i];
                size_t j = i;

                for (; j > 0 && sc->cross[j - 1] > c; j--)
                    sc->cross[j] = sc->cross[j - 1];
                sc->cross[j] = c;
            }
        for (size_t i = 0; i + 1 < n; i += 2) {
            int xa = first_index(gt[0], gt[1], 0, W, sc->cross[i], GE);
            int xb = first_index(gt[0], gt[1], 0, W, sc->cross[i + 1], GE);

            if (xa < cx0)
                xa = cx0;
            if (xb > cx1)
                xb = cx1;
            if (xa < xb && span_push(out, y, xa, xb, local, max_span_px) != 0)
                return -1;
        }
    }
    return 0;
}

/* the owned pixel rectangle [*x0, *x1) x [*y0, *y1) of a W x H block: centres with own[0] <= px < own[2] and
 * own[1] < py <= own[3] (north up, checked by the callers) */
NO_CONTRACT void gcn10_owned_window(const double gt[6], int W, int H, const double own[4], int *x0, int *x1, int *y0,
                                    int *y1)
{
    *x0 = first_index(gt[0], gt[1], 0, W, own[0], GE);
    *x1 = first_index(gt[0], gt[1], 0, W, own[2], GE);
    *y0 = first_index(gt[3], gt[5], 0, H, own[3], LE);
    *y1 = first_index(gt[3], gt[5], 0, H, own[1], LE);
}

NO_CONTRACT int gcn10_zones_build_plan(const gcn10_zones *z, const double gt[6], int W, int H, const double own[4],
                                       uint32_t max_span_px, uint32_t max_item_px, gcn10_zone_plan *out, char *err,
                                       size_t errcap)
{
    struct scratch sc;
    struct span_list spans = { NULL, 0, 0 };
    int oy0 = 0, oy1 = H - 1, ox0 = 0, ox1 = W, rc = -1;
    size_t local_cap = 0, pixels_cap = 0;

    memset(&sc, 0, sizeof sc);
    memset(out, 0, sizeof *out);
    if (W <= 0 || H <= 0 || !(gt[1] > 0.0) || !(gt[5] < 0.0) || gt[2] != 0.0 || gt[4] != 0.0 || !isfinite(gt[0]) ||
        !isfinite(gt[3]) || !isfinite(gt[1]) || !isfinite(gt[5])) {
        snprintf(err, errcap, "zones need a north-up block without rotation (%d x %d, pixel %g x %g)", W, H, gt[1], gt[5]);
        return -1;
    }
    bounds_of(&max_span_px, &max_item_px);
    if (own) {
        gcn10_owned_window(gt, W, H, own, &ox0, &ox1, &oy0, &oy1);
        oy1--;
    }
    for (int zi = 0; zi < z->n && ox0 < ox1 && oy0 <= oy1; zi++) {
        const double *b = z->bbox[zi];
        const size_t before = spans.n;
        int ry0, ry1, cx0, cx1;

        if (z->ring_first[zi + 1] == z->ring_first[zi])
            continue;
        /* the rows and columns whose centres lie in the record's bounding box, within the owned ones */
        ry0 = first_index(gt[3], gt[5], 0, H, b[3], LE);
        ry1 = first_index(gt[3], gt[5], 0, H, b[1], LT) - 1;
        cx0 = first_index(gt[0], gt[1], 0, W, b[0], GE);
        cx1 = first_index(gt[0], gt[1], 0, W, b[2], GT);
        if (ry0 < oy0)
            ry0 = oy0;
        if (ry1 > oy1)
            ry1 = oy1;
        if (ry0 > ry1 || (cx0 > ox0 ? cx0 : ox0) >= (cx1 < ox1 ? cx1 : ox1))
            continue;
        if (scan_zone(z, zi, gt, W, ry0, ry1, ox0, ox1, out->n_local, max_span_px, &sc, &spans) != 0)
            goto oom;
        if (spans.n == before)
            continue;
        if (grow((void **)&out->local_zone, &local_cap, (size_t)out->n_local + 1, sizeof *out->local_zone) != 0 ||
            grow((void **)&out->local_pixels, &pixels_cap, (size_t)out->n_local + 1, sizeof *out->local_pixels) != 0)
            goto oom;
        out->local_zone[out->n_local] = zi;
        out->local_pixels[out->n_local] = 0;
        for (size_t i = before; i < spans.n; i++)
            out->local_pixels[out->n_local] += (uint64_t)(spans.v[i].x1 - spans.v[i].x0);
        out->n_local++;
    }
    if (items_of(spans.v, spans.n, max_item_px, &out->items, &out->n_items) != 0)
        goto oom;
    out->spans = spans.v;
    out->n_spans = spans.n;
    spans.v = NULL;
    rc = 0;
oom:
    if (rc != 0) {
        snprintf(err, errcap, "out of memory for the spans of the zones");
        gcn10_zone_plan_free(out);
    }
    free(spans.v);
    free(sc.edges);
    free(sc.head);
    free(sc.active);
    free(sc.cross);
    return rc;
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* spans cut at the depth changes of rainfall rasters (config keys "zone_rain" and "zone_rains")                     */
/* ---------------------------------------------------------------------------------------------------------------- */

void gcn10_zone_rain_plan_free(gcn10_zone_rain_plan *p)
{
    free(p->rain_pixels);
    free(p->rain_sum);
    free(p->spans);
    free(p->items);
    memset(p, 0, sizeof *p);
}

void gcn10_zone_rains_plan_free(gcn10_zone_rains_plan *p)
{
    free(p->rain_pixels);
    for (int j = 0; j < GCN10_MAX_RAINS; j++)
        free(p->rain_sum[j]);
    free(p->spans);
    free(p->items);
    memset(p, 0, sizeof *p);
}

/* a piece of a source span under one tuple: layer 0 in t[0], the bytes from k on zero */
struct rain_piece {
    int32_t y, x0, x1;
    uint8_t t[8];
};

struct rain_pieces {
    struct rain_piece *v;
    size_t n, cap;
};

static int rain_piece_push(struct rain_pieces *l, int32_t y, int32_t x0, int32_t x1, const uint8_t t[8])
{
    if (l->n == l->cap) {
        const size_t cap = l->cap ? l->cap * 2 : 1024;
        struct rain_piece *g = realloc(l->v, cap * sizeof *g);

        if (!g)
            return -1;
        l->v = g;
        l->cap = cap;
    }
    l->v[l->n] = (struct rain_piece){ y, x0, x1, { 0 } };
    memcpy(l->v[l->n++].t, t, 8);
    return 0;
}

struct rains_items {
    gcn10_zone_rains_item *v;
    size_t n, cap;
};

static int rains_item_push(struct rains_items *l, uint32_t first, uint32_t n, const uint8_t t[8])
{
    if (l->n == l->cap) {
        const size_t cap = l->cap ? l->cap * 2 : 256;
        gcn10_zone_rains_item *g = realloc(l->v, cap * sizeof *g);

        if (!g)
            return -1;
        l->v = g;
        l->cap = cap;
    }
    l->v[l->n] = (gcn10_zone_rains_item){ first, n, { 0 } };
    memcpy(l->v[l->n++].table, t, 8);
    return 0;
}

int gcn10_zone_rains_cut(const gcn10_zone_plan *plan, int W, int H, const int32_t *cellx, const int32_t *celly, int cx0,
                         int cy0, const uint8_t *const rain[], int k, int nx, int ny, uint32_t max_span_px,
                         uint32_t max_item_px, gcn10_zone_rains_plan *out)
{
    struct rain_pieces pieces = { NULL, 0, 0 };
    struct span_list cut = { NULL, 0, 0 };
    struct rains_items items = { NULL, 0, 0 };
    struct rain_piece *sorted = NULL;
    size_t sorted_cap = 0;
    int32_t *next = NULL;       /* next[x]: the first column after x whose entry of cellx differs from cellx[x] */
    bool layers = rain != NULL;
    int rc = -1;

    memset(out, 0, sizeof *out);
    if (W <= 0 || H <= 0 || plan->n_local < 0 || plan->n_spans > 0xffffffffu || k < 1 || k > GCN10_MAX_RAINS)
        return -1;
    bounds_of(&max_span_px, &max_item_px);
    out->n_local = plan->n_local;
    out->k = k;
    out->rain_pixels = calloc((size_t)plan->n_local + 1, sizeof *out->rain_pixels);
    if (!out->rain_pixels)
        goto done;
    for (int j = 0; j < k; j++) {
        out->rain_sum[j] = calloc((size_t)plan->n_local + 1, sizeof *out->rain_sum[j]);
        if (!out->rain_sum[j])
            goto done;
        layers = layers && rain[j] != NULL;
    }
    if (!cellx || !celly || !layers || nx <= 0 || ny <= 0 || plan->n_spans == 0) {
        rc = 0;                 /* a block without rain cells, or without zones */
        goto done;
    }
    next = malloc((size_t)W * sizeof *next);
    if (!next)
        goto done;
    next[W - 1] = W;
    for (int x = W - 2; x >= 0; x--)
        next[x] = cellx[x + 1] == cellx[x] ? next[x + 1] : x + 1;

    for (size_t i = 0; i < plan->n_spans;) {
        const int32_t zone = plan->spans[i].zone;
        size_t j = i;

        /* the pieces of the zone, in the order of its spans: (y, x0) */
        pieces.n = 0;
        for (; j < plan->n_spans && plan->spans[j].zone == zone; j++) {
            const gcn10_zone_span *sp = &plan->spans[j];
            int32_t run0 = 0, run1 = 0;         /* the open run [run0, run1) of tuple runt; empty: none */
            uint8_t runt[8] = { 0 };
            size_t row;
            int64_t cy;

            if (sp->y < 0 || sp->y >= H || sp->x0 < 0 || sp->x1 > W || sp->x0 >= sp->x1 || zone < 0 ||
                zone >= plan->n_local)
                goto done;
            cy = (int64_t)celly[sp->y] + cy0;
            if (celly[sp->y] < 0 || cy >= ny)
                continue;
            row = (size_t)cy * (size_t)nx;
            for (int32_t x = sp->x0; x <= sp->x1;) {
                const int32_t end = x < sp->x1 ? (next[x] < sp->x1 ? next[x] : sp->x1) : x + 1;
                const int64_t cx = x < sp->x1 ? (int64_t)cellx[x] + cx0 : -1;
                const bool in = x < sp->x1 && cellx[x] >= 0 && cx < nx;
                uint8_t t[8] = { 0 };

                for (int m = 0; in && m < k; m++)
                    t[m] = rain[m][row + (size_t)cx];
                if (in && run1 > run0 && run1 == x && memcmp(t, runt, 8) == 0) {
                    run1 = end;         /* a neighbouring cell of equal tuple */
                }
                else {
                    if (run1 > run0) {
                        if (rain_piece_push(&pieces, sp->y, run0, run1, runt) != 0)
                            goto done;
                        out->rain_pixels[zone] += (uint64_t)(run1 - run0);
                        for (int m = 0; m < k; m++)
                            out->rain_sum[m][zone] += (uint64_t)(run1 - run0) * runt[m];
                    }
                    run0 = run1 = 0;
                    if (in) {
                        run0 = x;
                        run1 = end;
                        memcpy(runt, t, 8);
                    }
                }
                x = end;
            }
        }
        i = j;
        if (pieces.n == 0)
            continue;

        /* a counting sort per layer, the last first, keeps (y, x0) within a tuple and leaves the tuples in
         * lexicographic order; an even number of passes ends in pieces.v, an odd one in sorted */
        if (grow((void **)&sorted, &sorted_cap, pieces.n, sizeof *sorted) != 0)
            goto done;
        {
            struct rain_piece *src = pieces.v, *dst = sorted;

            for (int m = k - 1; m >= 0; m--) {
                size_t count[257] = { 0 };
                struct rain_piece *tmp;

                for (size_t q = 0; q < pieces.n; q++)
                    count[src[q].t[m] + 1]++;
                for (int b = 0; b < 256; b++)
                    count[b + 1] += count[b];
                for (size_t q = 0; q < pieces.n; q++)
                    dst[count[src[q].t[m]]++] = src[q];
                tmp = src;
                src = dst;
                dst = tmp;
            }

            /* the zone's spans, never longer than max_span_px, and items of one tuple with at most max_item_px pixels */
            for (size_t q = 0; q < pieces.n;) {
                const uint8_t *t = src[q].t;
                size_t first = cut.n;
                uint64_t px = 0;

                for (; q < pieces.n && memcmp(src[q].t, t, 8) == 0; q++) {
                    const size_t before = cut.n;

                    if (span_push(&cut, src[q].y, src[q].x0, src[q].x1, zone, max_span_px) != 0)
                        goto done;
                    for (size_t m = before; m < cut.n; m++) {
                        const uint64_t len = (uint64_t)(cut.v[m].x1 - cut.v[m].x0);

                        if (m > first && px + len > max_item_px) {
                            if (rains_item_push(&items, (uint32_t)first, (uint32_t)(m - first), t) != 0)
                                goto done;
                            first = m;
                            px = 0;
                        }
                        px += len;
                    }
                }
                if (cut.n > 0xffffffffu || rains_item_push(&items, (uint32_t)first, (uint32_t)(cut.n - first), t) != 0)
                    goto done;
            }
        }
    }
    out->spans = cut.v;
    out->n_spans = cut.n;
    out->items = items.v;
    out->n_items = items.n;
    cut.v = NULL;
    items.v = NULL;
    rc = 0;
done:
    if (rc != 0)
        gcn10_zone_rains_plan_free(out);
    free(pieces.v);
    free(cut.v);
    free(items.v);
    free(sorted);
    free(next);
    return rc;
}

/* one layer: the same walk, its items and sums in the one-raster form */
int gcn10_zone_rain_cut(const gcn10_zone_plan *plan, int W, int H, const int32_t *cellx, const int32_t *celly, int cx0,
                        int cy0, const uint8_t *rain, int nx, int ny, uint32_t max_span_px, uint32_t max_item_px,
                        gcn10_zone_rain_plan *out)
{
    gcn10_zone_rains_plan many;

    memset(out, 0, sizeof *out);
    if (gcn10_zone_rains_cut(plan, W, H, cellx, celly, cx0, cy0, &rain, 1, nx, ny, max_span_px, max_item_px, &many) != 0)
        return -1;
    out->items = many.n_items ? malloc(many.n_items * sizeof *out->items) : NULL;
    if (many.n_items && !out->items) {
        gcn10_zone_rains_plan_free(&many);
        return -1;
    }
    for (size_t i = 0; i < many.n_items; i++)
        out->items[i] = (gcn10_zone_rain_item){ many.items[i].first_span, many.items[i].n_spans, many.items[i].table[0], 0 };
    out->n_local = many.n_local;
    out->rain_pixels = many.rain_pixels;
    out->rain_sum = many.rain_sum[0];
    out->n_spans = many.n_spans;
    out->n_items = many.n_items;
    out->spans = many.spans;
    free(many.items);
    return 0;
}
