/* rain_san_main.c -- the unit parser and the table builder of the rainfall raster (csrc/host/runoff.c:
 * gcn10_parse_rain_unit, gcn10_rain_tables) as a program of its own, built with AddressSanitizer + UBSan by
 * tests/test_rain_host.py.
 *
 *   rain_san <rain_unit text>...
 *
 * prints, per text, "bad" for one gcn10_parse_rain_unit refuses, else "unit <unit> <lambda> | <q[1][100]> <q[128][100]>
 * <q[255][100]> <q[255][50]> <sum of all entries>".  The 256 tables are built in a heap block of exactly 256 x 256
 * values, so that a write beyond it is seen; a refused text must leave unit and lambda as they were.  The exit status
 * is 1 when a text was refused, 3 when a refused text wrote or a table broke its rule (q[b][0] = q[b][255] = 0, table 0
 * all zero). */
#include "gcn10_host.h"

#include <stdio.h>
#include <stdlib.h>

int main(int argc, char **argv)
{
    int status = 0;

    for (int a = 1; a < argc; a++) {
        double unit = -7.0, lambda = -7.0;
        uint16_t (*q)[256] = malloc(256 * sizeof *q);
        unsigned long long sum = 0;

        if (!q)
            return 2;
        if (gcn10_parse_rain_unit(argv[a], &unit, &lambda) != 0) {
            if (unit != -7.0 || lambda != -7.0)
                status = 3;
            printf("bad\n");
            if (status == 0)
                status = 1;
        }
        else {
            gcn10_rain_tables(unit, lambda, q);
            for (int b = 0; b < 256; b++) {
                if (q[b][0] != 0 || q[b][255] != 0)
                    status = 3;
                for (int v = 0; v < 256; v++) {
                    sum += q[b][v];
                    if (b == 0 && q[b][v] != 0)
                        status = 3;
                }
            }
            printf("unit %.17g %.17g | %u %u %u %u %llu\n", unit, lambda, (unsigned)q[1][100], (unsigned)q[128][100],
                   (unsigned)q[255][100], (unsigned)q[255][50], sum);
        }
        free(q);
    }
    return status;
}
