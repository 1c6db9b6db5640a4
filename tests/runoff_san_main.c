/* runoff_san_main.c -- the host functions of the design storm (csrc/host/runoff.c) as a program of their own, built
 * with AddressSanitizer + UBSan by tests/test_runoff_host.py.
 *
 *   runoff_san <storm text> [<s> <n> <sw>]...
 *
 * prints "bad" for a text gcn10_parse_storm refuses (exit status 1), else one line "storm <P> <lambda>", one line with
 * the 256 values of gcn10_runoff_table and one line "cn <value>" per triple by gcn10_runoff_cn. */
#include "gcn10_host.h"

#include <stdio.h>
#include <stdlib.h>

int main(int argc, char **argv)
{
    double P, lambda;
    uint16_t *q;

    if (argc < 2 || gcn10_parse_storm(argv[1], &P, &lambda) != 0) {
        printf("bad\n");
        return 1;
    }
    q = malloc(256 * sizeof *q);        /* on the heap, exactly 256 entries: an index beyond them is seen */
    if (!q)
        return 2;
    gcn10_runoff_table(P, lambda, q);
    printf("storm %.17g %.17g\n", P, lambda);
    for (int v = 0; v < 256; v++)
        printf("%u%c", (unsigned)q[v], v < 255 ? ' ' : '\n');
    for (int i = 2; i + 2 < argc; i += 3)
        printf("cn %d\n", gcn10_runoff_cn(strtoull(argv[i], NULL, 10), strtoull(argv[i + 1], NULL, 10),
                                          strtoull(argv[i + 2], NULL, 10), q));
    free(q);
    return 0;
}
