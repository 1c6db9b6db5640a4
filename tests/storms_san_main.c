/* storms_san_main.c -- the parser of several design storms (csrc/host/runoff.c: gcn10_parse_storms) as a program of its
 * own, built with AddressSanitizer + UBSan by tests/test_storms_host.py.
 *
 *   storms_san <storms text>...
 *
 * prints, per text, "bad" for one gcn10_parse_storms refuses, else "storms <k> <lambda> <P1> ... <Pk> | <N1> ... <Nk>"
 * with N = q[100] of gcn10_runoff_table.  The depths are parsed into a heap block of exactly GCN10_MAX_STORMS doubles
 * preset to a marker: a write beyond it is seen, and a refused text must leave it as it was.  The exit status is 1 when
 * a text was refused, 3 when a refused text wrote. */
#include "gcn10_host.h"

#include <stdio.h>
#include <stdlib.h>

int main(int argc, char **argv)
{
    int status = 0;

    for (int a = 1; a < argc; a++) {
        double *P = malloc(GCN10_MAX_STORMS * sizeof *P), lambda = -7.0;
        uint16_t *q = malloc(256 * sizeof *q);
        int k = -7;

        if (!P || !q)
            return 2;
        for (int i = 0; i < GCN10_MAX_STORMS; i++)
            P[i] = -7.0;
        if (gcn10_parse_storms(argv[a], P, &k, &lambda) != 0) {
            for (int i = 0; i < GCN10_MAX_STORMS; i++)
                if (P[i] != -7.0)
                    status = 3;
            if (k != -7 || lambda != -7.0)
                status = 3;
            printf("bad\n");
            if (status == 0)
                status = 1;
        }
        else {
            printf("storms %d %.17g", k, lambda);
            for (int i = 0; i < k; i++)
                printf(" %.17g", P[i]);
            printf(" |");
            for (int i = 0; i < k; i++) {
                gcn10_runoff_table(P[i], lambda, q);
                printf(" %u", (unsigned)q[100]);
            }
            printf("\n");
        }
        free(P);
        free(q);
    }
    return status;
}
