/* tiff_san_main.c -- stand-alone driver of the GeoTIFF module (gcn10_amd/csrc/host/tiff_*.c, with pool.c), built by
 * tests/test_tiff_san.py with -fsanitize=address,undefined and leak detection.
 *
 *   tiff_san <directory>
 *
 * <directory>/layouts.txt names small TIFF files of the 13 x 11 raster of tests/test_tiff_pins.py ("<file> <what the
 * planner answers>"), <directory>/fuzz.txt damaged files.  The program
 *   - writes 600 x 300 rasters, plain and as a COG, through each of the three puts; finishes them, reopens every
 *     directory and checks the pixels; aborts one; finishes one after a refused put and one after a put that marks the
 *     writer failed;
 *   - reads the single-pixel, edge and full windows of every layout without and with an I/O pool, and plans them;
 *   - opens, reads and plans every damaged file, whatever comes of it.
 * Prints "tiff_san: N cases ok" (exit 0), or the first failed check (exit 1). */
#include "tiff_internal.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

/* read_chunk()'s decode buffers belong to their thread and live as long as it does; a pool thread that ends leaves
 * them behind, which is how the product is and no business of this program */
const char *__lsan_default_suppressions(void);
const char *__lsan_default_suppressions(void)
{
    return "leak:read_chunk\n";
}

static long n_cases;
static char err[512];

#define CHECK(cond, ...) \
    do { \
        if (!(cond)) { \
            fprintf(stderr, "tiff_san: %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, " [%s]\n", err); \
            exit(1); \
        } \
    } while (0)

/* ---- writer ---- */

enum { XS = 600, YS = 300, N_LEVELS = 2, T = 256 };
static const int across[3] = { 3, 2, 1 }, down[3] = { 2, 1, 1 };
static const double gt[6] = { 10.0, 0.5, 0.0, 50.0, 0.0, -0.5 };
static uint8_t blob[3][6][1024];
static uint32_t blob_len[3][6];

static uint8_t tile_value(int level, int i)
{
    return (uint8_t)(1 + 10 * level + i);
}

static void make_blobs(void)
{
    static uint8_t px[T * T];

    for (int level = 0; level <= N_LEVELS; level++)
        for (int i = 0; i < across[level] * down[level]; i++) {
            memset(px, tile_value(level, i), sizeof px);
            blob_len[level][i] = (uint32_t)gcn10_deflate_tile(px, T, T, T, 1, blob[level][i], sizeof blob[level][i]);
            CHECK(blob_len[level][i] > 0, "level %d tile %d", level, i);
        }
}

/* every tile of a level through put `kind` (0 tile, 1 tiles, 2 extent); 0 when every put was taken */
static int fill_level(gcn10_tiff_writer *w, int level, int kind)
{
    gcn10_tiff_writer *v = gcn10_tiff_level(w, level);
    const int n = across[level] * down[level];
    int tx[6], ty[6], rc = 0;
    const void *ptr[6];
    uint32_t rel[6], len[6], at = 0;
    static uint8_t extent[8192] __attribute__((aligned(4096)));

    for (int i = 0; i < n; i++) {
        tx[i] = i % across[level];
        ty[i] = i / across[level];
        ptr[i] = blob[level][i];
        len[i] = blob_len[level][i];
        rel[i] = at;
        memcpy(extent + at, blob[level][i], len[i]);
        at = (at + len[i] + 15u) & ~15u;
    }
    CHECK(at <= 4096, "extent of level %d", level);
    if (kind == 0)
        for (int i = 0; i < n; i++)
            rc |= gcn10_tiff_put_tile(v, tx[i], ty[i], ptr[i], len[i]);
    else if (kind == 1)
        rc = gcn10_tiff_put_tiles(v, n, tx, ty, ptr, len);
    else
        rc = gcn10_tiff_put_extent(v, extent, rel[n - 1] + len[n - 1], n, tx, ty, rel, len);
    return rc;
}

static void check_written(const char *path, int n_levels)
{
    static uint8_t px[XS * YS];

    for (int level = 0; level <= n_levels; level++) {
        int why = 0, xs, ys;
        double g[6];
        struct gcn10_tiff *t = gcn10_tiff_open_reader_ifd(path, level, &why, err, sizeof err);

        CHECK(t, "%s level %d", path, level);
        gcn10_tiff_reader_info(t, &xs, &ys, g);
        CHECK(xs == gcn10_level_dim(XS, level) && ys == gcn10_level_dim(YS, level), "%s level %d: %dx%d", path, level, xs, ys);
        CHECK(gcn10_tiff_reader_has_next(t) == (level < n_levels), "%s level %d", path, level);
        CHECK(gcn10_tiff_read_window(t, 0, 0, xs, ys, px, (size_t)xs, err, sizeof err) == 0, "%s level %d", path, level);
        for (int y = 0; y < ys; y++)
            for (int x = 0; x < xs; x++)
                CHECK(px[y * xs + x] == tile_value(level, y / T * across[level] + x / T), "%s level %d at %d,%d", path,
                      level, x, y);
        gcn10_tiff_close_reader(t);
    }
    CHECK(gcn10_tiff_open_reader_ifd(path, n_levels + 1, NULL, err, sizeof err) == NULL, "%s", path);
}

static gcn10_tiff_writer *create(const char *path, int cog, int direct)
{
    gcn10_tiff_writer *w = cog ? gcn10_tiff_create_cog(path, XS, YS, gt, NULL, N_LEVELS, err, sizeof err)
                               : gcn10_tiff_create(path, XS, YS, gt, NULL, err, sizeof err);

    CHECK(w, "%s", path);
    if (cog) {
        CHECK(gcn10_tiff_set_nodata(w, 255) == 0, "%s", path);
        CHECK(gcn10_tiff_reserve_metadata(w, 256) == 0, "%s", path);
    }
    if (direct)
        gcn10_tiff_set_direct(w, true);         /* a file system may refuse it */
    return w;
}

static void writer_cases(const char *dir)
{
    char path[1024], part[1040];

    snprintf(path, sizeof path, "%s/w.tif", dir);
    snprintf(part, sizeof part, "%s.part", path);
    make_blobs();
    for (int cog = 0; cog <= 1; cog++) {
        for (int kind = 0; kind < 3; kind++) {
            for (int direct = 0; direct <= 1; direct++) {       /* written, finished, every level read back */
                gcn10_tiff_writer *w = create(path, cog, direct);

                for (int level = cog ? N_LEVELS : 0; level >= 0; level--)
                    CHECK(fill_level(w, level, kind) == 0, "cog %d put %d level %d", cog, kind, level);
                if (cog)
                    CHECK(gcn10_tiff_set_metadata_xml(w, "<GDALMetadata>\n</GDALMetadata>\n") == 0, "cog %d", cog);
                CHECK(gcn10_tiff_finish(w, err, sizeof err) == 0, "cog %d put %d", cog, kind);
                check_written(path, cog ? N_LEVELS : 0);
                unlink(path);
                n_cases++;
            }
            {                                                   /* aborted half way: no file, no .part */
                gcn10_tiff_writer *w = create(path, cog, 0);

                CHECK(fill_level(w, cog ? N_LEVELS : 0, kind) == 0, "cog %d put %d", cog, kind);
                gcn10_tiff_abort(w);
                CHECK(access(path, F_OK) != 0 && access(part, F_OK) != 0, "cog %d put %d", cog, kind);
                n_cases++;
            }
            {                                                   /* finished with a tile missing */
                gcn10_tiff_writer *w = create(path, cog, 0);

                if (cog)
                    CHECK(fill_level(w, N_LEVELS, kind) == 0, "cog %d put %d", cog, kind);
                CHECK(gcn10_tiff_finish(w, err, sizeof err) == -1 && strstr(err, "was never written"), "cog %d put %d", cog, kind);
                CHECK(access(path, F_OK) != 0 && access(part, F_OK) != 0, "cog %d put %d", cog, kind);
                n_cases++;
            }
            {                                                   /* finished after a put with a tile outside the grid */
                gcn10_tiff_writer *w = create(path, cog, 0);
                int tx = 3, ty = 0, rc;
                const void *ptr = blob[0][0];
                uint32_t rel = 0;

                for (int level = cog ? N_LEVELS : 1; level >= 1 && cog; level--)
                    CHECK(fill_level(w, level, kind) == 0, "cog %d put %d level %d", cog, kind, level);
                rc = kind == 0 ? gcn10_tiff_put_tile(w, tx, ty, ptr, blob_len[0][0])
                   : kind == 1 ? gcn10_tiff_put_tiles(w, 1, &tx, &ty, &ptr, &blob_len[0][0])
                               : gcn10_tiff_put_extent(w, ptr, blob_len[0][0], 1, &tx, &ty, &rel, &blob_len[0][0]);
                CHECK(rc == -1, "cog %d put %d", cog, kind);
                CHECK(fill_level(w, 0, kind) == 0, "cog %d put %d", cog, kind);
                rc = gcn10_tiff_finish(w, err, sizeof err);
                if (kind == 1) {                                /* the batch put marks the writer failed */
                    CHECK(rc == -1 && strstr(err, "write error on ") && access(path, F_OK) != 0, "cog %d", cog);
                }
                else {
                    CHECK(rc == 0, "cog %d put %d", cog, kind);
                    check_written(path, cog ? N_LEVELS : 0);
                    unlink(path);
                }
                n_cases++;
            }
        }
    }
}

/* ---- reader ---- */

enum { W = 13, H = 11 };
static const int windows[][4] = { { 0, 0, W, H }, { W - 1, H - 1, 1, 1 }, { 0, 0, 1, 1 }, { W - 1, 0, 1, H },
                                  { 0, H - 1, W, 1 }, { 0, 0, 4, 3 }, { 4, 3, 4, 3 }, { 12, 9, 1, 2 }, { 3, 2, 2, 2 },
                                  { 0, 9, W, 2 }, { 8, 0, 5, H } };
enum { N_WINDOWS = sizeof windows / sizeof windows[0] };

static void reader_cases(const char *dir, gcn10_pool *pool)
{
    char list[1024], name[256], path[1300];
    int plan_rc;
    FILE *f;

    snprintf(list, sizeof list, "%s/layouts.txt", dir);
    f = fopen(list, "r");
    CHECK(f, "%s", list);
    while (fscanf(f, "%255s %d", name, &plan_rc) == 2) {
        struct gcn10_tiff *t;

        snprintf(path, sizeof path, "%s/%s", dir, name);
        t = gcn10_tiff_open_reader(path, err, sizeof err);
        CHECK(t, "%s", path);
        for (int k = 0; k < N_WINDOWS; k++) {
            const int x = windows[k][0], y = windows[k][1], w = windows[k][2], h = windows[k][3];
            struct gcn10_read_plan plan = { 0 };
            uint8_t px[W * H];
            int rc;

            for (int with_pool = 0; with_pool <= 1; with_pool++) {
                memset(px, 0xEE, sizeof px);
                CHECK(gcn10_tiff_read_window_mt(t, x, y, w, h, px, (size_t)w, with_pool ? pool : NULL, err, sizeof err) == 0,
                      "%s window %d", name, k);
                for (int j = 0; j < h; j++)
                    for (int i = 0; i < w; i++)
                        CHECK(px[j * w + i] == (uint8_t)((y + j) * W + x + i + 17), "%s window %d at %d,%d", name, k, i, j);
            }
            rc = gcn10_tiff_plan_window(t, x, y, w, h, 0, 0, GCN10_CODEC_DEFLATE | GCN10_CODEC_RAW | GCN10_CODEC_LZW,
                                        &plan, err, sizeof err);
            CHECK(rc == plan_rc && (rc != 0 || plan.covered == (uint64_t)w * h), "%s window %d: plan %d", name, k, rc);
            free(plan.chunks);
            CHECK(gcn10_tiff_read_window(t, x + 1, y, W, h, px, W, err, sizeof err) == -1 && strstr(err, "outside raster"),
                  "%s window %d", name, k);
        }
        gcn10_tiff_close_reader(t);
        n_cases++;
    }
    fclose(f);
}

static void fuzz_cases(const char *dir, gcn10_pool *pool)
{
    char list[1024], name[256], path[1300];
    static uint8_t px[1 << 20];
    FILE *f;

    snprintf(list, sizeof list, "%s/fuzz.txt", dir);
    f = fopen(list, "r");
    CHECK(f, "%s", list);
    while (fscanf(f, "%255s", name) == 1) {
        int why = 0, xs, ys;
        double g[6];
        struct gcn10_tiff *t;

        snprintf(path, sizeof path, "%s/%s", dir, name);
        t = gcn10_tiff_open_reader_ifd(path, 0, &why, err, sizeof err);
        n_cases++;
        if (!t)
            continue;
        gcn10_tiff_reader_info(t, &xs, &ys, g);
        if (xs > 0 && ys > 0 && (uint64_t)xs * (uint64_t)ys <= sizeof px) {
            struct gcn10_read_plan plan = { 0 };
            uint64_t index, off, count;

            gcn10_tiff_read_window_mt(t, 0, 0, xs, ys, px, (size_t)xs, (n_cases & 1) ? pool : NULL, err, sizeof err);
            gcn10_tiff_plan_window(t, 0, 0, xs, ys, 0, 0, GCN10_CODEC_DEFLATE | GCN10_CODEC_RAW | GCN10_CODEC_LZW, &plan,
                                   err, sizeof err);
            for (size_t i = 0; i < plan.n; i++)                 /* what is planned lies inside the file */
                CHECK(plan.chunks[i].file_off + plan.chunks[i].nbytes <= t->file_size, "%s chunk %zu", name, i);
            free(plan.chunks);
            gcn10_tiff_check_chunks(t, &index, &off, &count);
        }
        gcn10_tiff_close_reader(t);
    }
    fclose(f);
}

int main(int argc, char **argv)
{
    gcn10_pool *pool;

    if (argc != 2) {
        fprintf(stderr, "usage: tiff_san <directory>\n");
        return 2;
    }
    writer_cases(argv[1]);
    pool = gcn10_pool_create(3);
    CHECK(pool, "pool");
    reader_cases(argv[1], pool);
    fuzz_cases(argv[1], pool);
    gcn10_pool_destroy(pool);
    printf("tiff_san: %ld cases ok\n", n_cases);
    return 0;
}
