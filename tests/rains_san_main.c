/* rains_san_main.c -- the host side of several rainfall rasters in one run (config key "rains": gcn10_parse_rains and
 * gcn10_rains_cell of csrc/host/runoff.c, gcn10_rains_load of csrc/host/grid.c) as a program of its own, built with
 * AddressSanitizer + UBSan against the host library's sources by tests/test_rains_host.py.
 *
 *   rains_san parse <text>...           per text "bad", or "<k>" and the k names, each in brackets
 *   rains_san load <grid> <text>        the K rasters of <text> on <grid>: per raster "<j> <sum of bytes> <first> <last>",
 *                                       or "error <rc> <message>" (exit status 1) with every pointer NULL again
 *   rains_san cells <n>                 n random cells of 1 to 8 layers through gcn10_rains_cell, words, bytes and
 *                                       results in heap blocks of exactly their size, against a plain restatement of
 *                                       the cell rule; "cells ok", or exit status 3
 *
 * A refused text must leave copy, files and k as they were (exit status 3 otherwise). */
#include "gcn10_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static uint64_t state = 88172645463325252ull;

static uint64_t next(void)                  /* xorshift64 */
{
    state ^= state << 13;
    state ^= state >> 7;
    state ^= state << 17;
    return state;
}

/* the rule of gcn10_runoff_cn as include/gcn10_host.h states it */
static int plain_cn(uint64_t s, uint64_t n, uint64_t sw, const uint16_t *q)
{
    if (n == 0)
        return 255;
    if (sw == 0)
        return (int)((2 * s + n) / (2 * n));
    for (int c = 1; c <= 100; c++)
        if (n * (uint64_t)q[c] >= sw)
            return c;
    return 100;
}

static int do_parse(int argc, char **argv)
{
    int status = 0;

    for (int a = 2; a < argc; a++) {
        char *copy = (char *)argv;              /* a marker: a refused text leaves it */
        const char *files[GCN10_MAX_RAINS];
        int k = -7;

        for (int j = 0; j < GCN10_MAX_RAINS; j++)
            files[j] = argv[0];
        if (gcn10_parse_rains(argv[a], &copy, files, &k) != 0) {
            if (copy != (char *)argv || k != -7)
                return 3;
            for (int j = 0; j < GCN10_MAX_RAINS; j++)
                if (files[j] != argv[0])
                    return 3;
            printf("bad\n");
            status = 1;
            continue;
        }
        printf("%d", k);
        for (int j = 0; j < k; j++)
            printf(" [%s]", files[j]);
        printf("\n");
        free(copy);
    }
    return status;
}

static int do_load(const char *grid_text, const char *text)
{
    gcn10_grid g;
    char *copy = NULL, err[8192] = "";
    const char *files[GCN10_MAX_RAINS];
    uint8_t *out[GCN10_MAX_RAINS];
    int k = 0, rc;

    if (gcn10_parse_grid(grid_text, &g) != 0 || gcn10_parse_rains(text, &copy, files, &k) != 0)
        return 2;
    memset(out, 0xff, sizeof out);              /* not NULL: the call sets every pointer */
    rc = gcn10_rains_load(files, k, &g, out, err, sizeof err);
    if (rc != 0) {
        for (int j = 0; j < GCN10_MAX_RAINS; j++)
            if (out[j] != NULL)
                return 3;
        printf("error %d %s\n", rc, err);
        free(copy);
        return 1;
    }
    for (int j = 0; j < GCN10_MAX_RAINS; j++) {
        const size_t n = (size_t)g.nx * (size_t)g.ny;
        unsigned long long sum = 0;

        if ((out[j] != NULL) != (j < k))
            return 3;
        if (j >= k)
            continue;
        for (size_t c = 0; c < n; c++)
            sum += out[j][c];                   /* every byte of the block, and none behind it */
        printf("%d %llu %u %u\n", j + 1, sum, (unsigned)out[j][0], (unsigned)out[j][n - 1]);
        free(out[j]);
    }
    free(copy);
    return 0;
}

static int do_cells(long n_cells)
{
    uint16_t (*q)[256] = malloc(256 * sizeof *q);

    if (!q)
        return 2;
    gcn10_rain_tables(2.5, 0.05, q);
    for (long c = 0; c < n_cells; c++) {
        const int k = 1 + (int)(next() % GCN10_MAX_RAINS);
        uint64_t *words = malloc((size_t)(2 + k) * sizeof *words);
        uint8_t *bytes = malloc((size_t)k), *cn = malloc((size_t)k);

        if (!words || !bytes || !cn)
            return 2;
        words[1] = c % 7 == 0 ? 0 : 1 + next() % (c % 3 ? 1000 : (1ull << 36));
        words[0] = words[1] * (1 + next() % 100) - (words[1] ? next() % words[1] : 0);
        for (int j = 0; j < k; j++) {
            bytes[j] = (uint8_t)(c % 5 == 0 ? 0 : next());
            /* around n q[b][v] for some v, so that every c of the rule is met; and 0 */
            words[2 + j] = next() % 4 == 0 ? 0 : words[1] * q[bytes[j]][1 + next() % 100] + next() % 3;
            cn[j] = 7;
        }
        gcn10_rains_cell(words, k, bytes, (const uint16_t (*)[256])q, cn);
        for (int j = 0; j < k; j++)
            if (cn[j] != plain_cn(words[0], words[1], words[2 + j], q[bytes[j]])) {
                printf("cell %ld layer %d: %u\n", c, j, (unsigned)cn[j]);
                return 3;
            }
        free(words);
        free(bytes);
        free(cn);
    }
    free(q);
    printf("cells ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "parse"))
        return do_parse(argc, argv);
    if (argc == 4 && !strcmp(argv[1], "load"))
        return do_load(argv[2], argv[3]);
    if (argc == 3 && !strcmp(argv[1], "cells"))
        return do_cells(atol(argv[2]));
    return 2;
}
