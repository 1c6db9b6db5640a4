/* zone_rains_san_main.c -- gcn10_zone_rains_cut as a stand-alone program, for AddressSanitizer + UBSan
 * (tests/test_zone_rains_host.py builds it with zones.c and runs it; nothing is preloaded).
 *
 * The window, the four zones, the cell maps (7, 16, 100 and 1000 pixel cells), the truncations of the maps' valid range
 * and the three pairs of bounds are those of zone_rain_san_main.c; here every case has k = 1, 2, 3 or 8 layers of random
 * bytes, of few bytes (so that neighbouring cells share a tuple, or differ in the last layer only) or of one byte.  Every
 * cut is checked against a per-pixel model: each pixel of a zone that lies in a cell is named once, under its tuple,
 * bytes k..7 of a tuple are zero, the spans are sorted by (zone, tuple, y, x0) with tuples in lexicographic order, the
 * items are of one zone and one tuple and honour the bounds, and rain_pixels and the k sums per zone are the model's.
 * With k copies of one layer the cut is that of gcn10_zone_rain_cut with the byte repeated.  Exit 0 and "cases ok", or 1
 * with the first difference. */
#include "gcn10_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

enum { W = 203, H = 151, NZ = 4 };

static uint32_t rng_state = 4711u;
static uint32_t rnd(void)
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

static int in_zone(int z, int x, int y)
{
    const long dx = x - 70, dy = y - 60;

    switch (z) {
    case 0: return dx * dx + dy * dy < 55 * 55 && !(dx * dx + dy * dy < 20 * 20);
    case 1: return x >= 90 && x < 195 && y >= 50 && y < 140;
    case 2: return x >= 150 && x < W && y >= 5 && y < 80;
    default: return y >= 120 && y < 125 && x >= 4 + (y - 120) && x < 6 + (y - 120);
    }
}

static int fail(const char *what, int a, int b, int c)
{
    printf("FAILED: %s (%d, %d, %d)\n", what, a, b, c);
    return 1;
}

/* cell size, first and last valid entry -> map[n]; cells count from `first` */
static void make_map(int32_t *map, int n, int cell, int first, int last)
{
    for (int i = 0; i < n; i++)
        map[i] = i >= first && i <= last ? (i - first) / cell : -1;
}

static int run_case(const gcn10_zone_plan *plan, const int32_t *cellx, const int32_t *celly, int cx0, int cy0,
                    const uint8_t *const rain[], int k, int nx, int ny, uint32_t span_px, uint32_t item_px, int id)
{
    static uint8_t got[NZ][H][W][8];
    static uint8_t named[NZ][H][W];
    gcn10_zone_rains_plan cut;
    uint64_t pixels[NZ] = { 0 }, sum[8][NZ] = { { 0 } };
    size_t at = 0;

    if (gcn10_zone_rains_cut(plan, W, H, cellx, celly, cx0, cy0, rain, k, nx, ny, span_px, item_px, &cut) != 0)
        return fail("the cutter returned -1", id, 0, 0);
    memset(got, 0, sizeof got);
    memset(named, 0, sizeof named);
    if (cut.k != k)
        return fail("k", id, cut.k, k);
    for (size_t i = 0; i < cut.n_items; i++) {
        const gcn10_zone_rains_item *it = &cut.items[i];
        uint64_t px = 0;

        if (it->first_span != at || it->n_spans == 0)
            return fail("an item", id, (int)i, (int)it->first_span);
        for (int m = k; m < 8; m++)
            if (it->table[m] != 0)
                return fail("a byte beyond the layers is not zero", id, (int)i, m);
        for (size_t s = at; s < at + it->n_spans; s++) {
            const gcn10_zone_span *sp = &cut.spans[s];

            if (s >= cut.n_spans || sp->zone < 0 || sp->zone >= NZ || sp->y < 0 || sp->y >= H || sp->x0 < 0 ||
                sp->x0 >= sp->x1 || sp->x1 > W || sp->zone != cut.spans[at].zone)
                return fail("a span", id, (int)s, 0);
            if ((uint32_t)(sp->x1 - sp->x0) > (span_px ? span_px : 16384u))
                return fail("a span is longer than the bound", id, (int)s, sp->x1 - sp->x0);
            if (s > 0) {
                const gcn10_zone_span *b = sp - 1;
                const int t = s > at ? 0 : memcmp(cut.items[i - 1].table, it->table, 8);    /* < 0: the tuple rose */

                if (b->zone > sp->zone || (b->zone == sp->zone && (t > 0 || (t == 0 && (b->y > sp->y ||
                    (b->y == sp->y && b->x0 >= sp->x0))))))
                    return fail("the sort order", id, (int)s, 0);
            }
            for (int x = sp->x0; x < sp->x1; x++) {
                if (named[sp->zone][sp->y][x])
                    return fail("a pixel named twice", id, sp->y, x);
                named[sp->zone][sp->y][x] = 1;
                memcpy(got[sp->zone][sp->y][x], it->table, 8);
            }
            px += (uint64_t)(sp->x1 - sp->x0);
        }
        if (item_px && px > item_px && it->n_spans > 1)
            return fail("an item is larger than the bound", id, (int)i, (int)px);
        at += it->n_spans;
    }
    if (at != cut.n_spans)
        return fail("spans outside the items", id, (int)at, (int)cut.n_spans);
    for (int z = 0; z < NZ; z++)
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const int in = in_zone(z, x, y) && cellx && celly && cellx[x] >= 0 && celly[y] >= 0 &&
                               cellx[x] + cx0 < nx && celly[y] + cy0 < ny;

                if (named[z][y][x] != in)
                    return fail("a pixel", id, y, x);
                if (!in)
                    continue;
                pixels[z]++;
                for (int m = 0; m < k; m++) {
                    const uint8_t want = rain[m][(size_t)(celly[y] + cy0) * (size_t)nx + (size_t)(cellx[x] + cx0)];

                    if (got[z][y][x][m] != want)
                        return fail("the byte of a pixel", id, y, x);
                    sum[m][z] += want;
                }
            }
    if (cut.n_local != NZ)
        return fail("n_local", id, cut.n_local, 0);
    for (int z = 0; z < NZ; z++) {
        if (cut.rain_pixels[z] != pixels[z])
            return fail("the pixels of a zone", id, z, (int)cut.rain_pixels[z]);
        for (int m = 0; m < 8; m++)
            if (m < k ? cut.rain_sum[m][z] != sum[m][z] : cut.rain_sum[m] != NULL)
                return fail("the sum of a zone", id, z, m);
    }
    gcn10_zone_rains_plan_free(&cut);
    return 0;
}

/* k copies of one layer: the spans and items of the one-layer cut, the byte repeated */
static int same_as_one_layer(const gcn10_zone_plan *plan, const int32_t *cellx, const int32_t *celly, int cx0, int cy0,
                             const uint8_t *rain, int k, int nx, int ny, uint32_t span_px, uint32_t item_px, int id)
{
    const uint8_t *layers[8];
    gcn10_zone_rains_plan many;
    gcn10_zone_rain_plan one;
    int rc = 0;

    for (int m = 0; m < 8; m++)
        layers[m] = rain;
    if (gcn10_zone_rains_cut(plan, W, H, cellx, celly, cx0, cy0, layers, k, nx, ny, span_px, item_px, &many) != 0 ||
        gcn10_zone_rain_cut(plan, W, H, cellx, celly, cx0, cy0, rain, nx, ny, span_px, item_px, &one) != 0)
        return fail("a cutter returned -1", id, k, 0);
    if (many.n_spans != one.n_spans || many.n_items != one.n_items ||
        (one.n_spans && memcmp(many.spans, one.spans, one.n_spans * sizeof *one.spans) != 0))
        rc = fail("identical layers: the spans", id, (int)many.n_spans, (int)one.n_spans);
    for (size_t i = 0; !rc && i < one.n_items; i++) {
        if (many.items[i].first_span != one.items[i].first_span || many.items[i].n_spans != one.items[i].n_spans)
            rc = fail("identical layers: an item", id, (int)i, 0);
        for (int m = 0; !rc && m < 8; m++)
            if (many.items[i].table[m] != (m < k ? one.items[i].table : 0u))
                rc = fail("identical layers: a tuple", id, (int)i, m);
    }
    for (int z = 0; !rc && z < NZ; z++) {
        if (many.rain_pixels[z] != one.rain_pixels[z])
            rc = fail("identical layers: rain_pixels", id, z, 0);
        for (int m = 0; !rc && m < k; m++)
            if (many.rain_sum[m][z] != one.rain_sum[z])
                rc = fail("identical layers: rain_sum", id, z, m);
    }
    gcn10_zone_rains_plan_free(&many);
    gcn10_zone_rain_plan_free(&one);
    return rc;
}

int main(void)
{
    static const int cells[] = { 7, 16, 100, 1000 };
    static const int ks[] = { 1, 2, 3, 8 };
    static const uint32_t bounds[][2] = { { 0, 0 }, { 16, 16 }, { 5, 64 } };
    /* {first, last} valid entry of a map of n entries: n is added to a negative `last` */
    static const int trunc[][2] = { { 0, -1 }, { 9, -1 }, { 0, -12 }, { 30, -40 }, { 1, -0x7fff } /* all -1 */ };
    gcn10_zone_span *src = NULL;
    gcn10_zone_plan plan, built;
    size_t n = 0, cap = 0;
    int cases = 0;

    /* the zones' spans, sorted by (zone, y, x0), through the item builder (it splits at the default bound) */
    for (int z = 0; z < NZ; z++)
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W;) {
                int e = x;

                while (e < W && in_zone(z, e, y))
                    e++;
                if (e > x) {
                    if (n == cap) {
                        cap = cap ? 2 * cap : 1024;
                        src = realloc(src, cap * sizeof *src);
                        if (!src)
                            return 2;
                    }
                    src[n++] = (gcn10_zone_span){ y, x, e, z };
                    x = e;
                }
                else
                    x++;
            }
    if (gcn10_zone_items_build(src, n, 0, 0, &built) != 0)
        return 2;
    plan = built;
    plan.n_local = NZ;

    for (size_t c = 0; c < sizeof cells / sizeof *cells; c++)
        for (size_t tx = 0; tx < sizeof trunc / sizeof *trunc; tx++)
            for (size_t ty = 0; ty < sizeof trunc / sizeof *trunc; ty++)
                for (int kind = 0; kind < 3; kind++) {
                    const int cell = cells[c];
                    const int k = ks[(c + tx + 2 * ty + (size_t)kind) % 4];
                    const int lx = trunc[tx][1] < 0 ? W + trunc[tx][1] : trunc[tx][1];
                    const int ly = trunc[ty][1] < 0 ? H + trunc[ty][1] : trunc[ty][1];
                    const int cx0 = (int)(rnd() % 3u), cy0 = (int)(rnd() % 3u);
                    const int nx = cx0 + W / cell + 1, ny = cy0 + H / cell + 1;
                    int32_t *cellx = malloc(W * sizeof *cellx), *celly = malloc(H * sizeof *celly);
                    uint8_t *rain[8] = { NULL };
                    const uint32_t *b = bounds[(c + tx + ty + (size_t)kind) % 3];
                    int rc;

                    if (!cellx || !celly)
                        return 2;
                    make_map(cellx, W, cell, trunc[tx][0], lx);
                    make_map(celly, H, cell, trunc[ty][0], ly);
                    for (int m = 0; m < k; m++) {
                        rain[m] = malloc((size_t)nx * (size_t)ny);     /* exactly nx * ny: a byte beyond is a finding */
                        if (!rain[m])
                            return 2;
                        for (int i = 0; i < nx * ny; i++)
                            rain[m][i] = kind == 0 ? (uint8_t)(rnd() & 255u)
                                       : kind == 1 ? (uint8_t)((m == k - 1 ? rnd() % 3u : rnd() % 8u == 0u) * 100u)
                                                   : (uint8_t)(20 + m);
                    }
                    rc = run_case(&plan, cellx, celly, cx0, cy0, (const uint8_t *const *)rain, k, nx, ny, b[0], b[1], cases);
                    if (!rc)
                        rc = same_as_one_layer(&plan, cellx, celly, cx0, cy0, rain[0], k, nx, ny, b[0], b[1], cases);
                    free(cellx);
                    free(celly);
                    for (int m = 0; m < k; m++)
                        free(rain[m]);
                    if (rc)
                        return 1;
                    cases++;
                }
    /* a block that meets no cell: no maps at all; a plan without spans; k outside 1..8 */
    {
        const uint8_t one = 9;
        const uint8_t *layers[8] = { &one, &one, &one, &one, &one, &one, &one, &one };
        gcn10_zone_plan empty;
        gcn10_zone_rains_plan cut;

        if (run_case(&plan, NULL, NULL, 0, 0, layers, 3, 1, 1, 0, 0, cases++))
            return 1;
        memset(&empty, 0, sizeof empty);
        empty.n_local = 0;
        if (gcn10_zone_rains_cut(&empty, W, H, NULL, NULL, 0, 0, layers, 8, 1, 1, 0, 0, &cut) != 0 || cut.n_spans ||
            cut.n_items)
            return fail("an empty plan", 0, 0, 0);
        gcn10_zone_rains_plan_free(&cut);
        cases++;
        if (gcn10_zone_rains_cut(&plan, W, H, NULL, NULL, 0, 0, layers, 0, 1, 1, 0, 0, &cut) != -1 ||
            gcn10_zone_rains_cut(&plan, W, H, NULL, NULL, 0, 0, layers, 9, 1, 1, 0, 0, &cut) != -1 || cut.spans || cut.items)
            return fail("k outside 1..8", 0, 0, 0);
        cases++;
    }
    gcn10_zone_plan_free(&built);
    free(src);
    printf("%d cases ok\n", cases);
    return 0;
}
