/* zones_san_main.c -- stand-alone driver of the zone reader and the scan conversion (gcn10_amd/csrc/host/zones.c), built
 * by tests/test_zones_host.py with -fsanitize=address,undefined.
 *
 *   zones_san <file.shp | directory> gt0 gt1 gt3 gt5 W H
 *
 * A file: reads it, builds the plan of a W x H block and prints "zones N local L spans S items I pixels P" (exit 0), or
 * the reader's message (exit 1).  A directory: the same for every .shp in it, one "files N ok K refused M" line at the
 * end (exit 0): damaged files must end in a result or a message, never in a sanitizer report. */
#include "gcn10_host.h"

#include <dirent.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int one(const char *path, const double gt[6], int W, int H, int quiet)
{
    gcn10_zones z;
    gcn10_zone_plan plan;
    char err[1024] = "";
    uint64_t pixels = 0;

    if (gcn10_zones_open(path, NULL, &z, err, sizeof err) != 0) {
        if (!quiet)
            fprintf(stderr, "%s\n", err);
        return 1;
    }
    /* small bounds as well: the splitting and the item rule see every span */
    if (gcn10_zones_build_plan(&z, gt, W, H, NULL, 5, 9, &plan, err, sizeof err) != 0) {
        if (!quiet)
            fprintf(stderr, "%s\n", err);
        gcn10_zones_free(&z);
        return 1;
    }
    gcn10_zone_plan_free(&plan);
    if (gcn10_zones_build_plan(&z, gt, W, H, NULL, 0, 0, &plan, err, sizeof err) != 0) {
        if (!quiet)
            fprintf(stderr, "%s\n", err);
        gcn10_zones_free(&z);
        return 1;
    }
    for (size_t i = 0; i < plan.n_spans; i++) {
        const gcn10_zone_span *s = &plan.spans[i];

        if (s->y < 0 || s->y >= H || s->x0 < 0 || s->x0 >= s->x1 || s->x1 > W || s->zone < 0 || s->zone >= plan.n_local) {
            fprintf(stderr, "%s: span %zu outside the block\n", path, i);
            abort();
        }
        pixels += (uint64_t)(s->x1 - s->x0);
    }
    if (!quiet)
        printf("zones %d local %d spans %zu items %zu pixels %llu\n", z.n, plan.n_local, plan.n_spans, plan.n_items,
               (unsigned long long)pixels);
    gcn10_zone_plan_free(&plan);
    gcn10_zones_free(&z);
    return 0;
}

int main(int argc, char **argv)
{
    double gt[6] = { 0, 0, 0, 0, 0, 0 };
    DIR *d;
    int W, H;

    if (argc != 8) {
        fprintf(stderr, "usage: zones_san <file.shp | directory> gt0 gt1 gt3 gt5 W H\n");
        return 2;
    }
    gt[0] = atof(argv[2]);
    gt[1] = atof(argv[3]);
    gt[3] = atof(argv[4]);
    gt[5] = atof(argv[5]);
    W = atoi(argv[6]);
    H = atoi(argv[7]);
    d = opendir(argv[1]);
    if (d) {
        struct dirent *e;
        int n = 0, ok = 0;

        while ((e = readdir(d)) != NULL) {
            const size_t len = strlen(e->d_name);
            char path[4096];

            if (len < 4 || strcmp(e->d_name + len - 4, ".shp") != 0)
                continue;
            snprintf(path, sizeof path, "%s/%s", argv[1], e->d_name);
            n++;
            ok += one(path, gt, W, H, 1) == 0;
        }
        closedir(d);
        printf("files %d ok %d refused %d\n", n, ok, n - ok);
        return 0;
    }
    return one(argv[1], gt, W, H, 0);
}
