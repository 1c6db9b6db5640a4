/* runoff_bytes_san_main.c -- gcn10_runoff_bytes, gcn10_parse_runoff_unit and gcn10_runoff_unit_of as a stand-alone
 * program, for AddressSanitizer + UBSan (tests/test_runoff_raster_host.py builds it with runoff.c and runs it; nothing
 * is preloaded).
 *
 * Without arguments: the byte tables of random 16-bit tables and of gcn10_rain_tables for u in {1, 13, 100, 250, 65000}
 * between guard bytes, every entry against the integer rule restated here; the unit that never saturates; the parser on
 * texts that are refused and texts that are taken.  "cases ok" and exit 0, or the first difference and exit 1.
 * With one argument: the parser on that text -- "<u>" and exit 0, or "bad" and exit 1. */
#include "gcn10_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

enum { GUARD = 64 };

static uint32_t rng_state = 2463534242u;
static uint32_t rnd(void)
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

static int check_tables(uint16_t (*q)[256], unsigned u, const char *what)
{
    uint8_t *buf = malloc(2 * GUARD + 65536);
    uint8_t (*t)[256];

    if (!buf)
        return 1;
    memset(buf, 0xA5, 2 * GUARD + 65536);
    t = (uint8_t (*)[256])(buf + GUARD);
    gcn10_runoff_bytes(q, u, t);
    for (int i = 0; i < GUARD; i++)
        if (buf[i] != 0xA5 || buf[GUARD + 65536 + i] != 0xA5) {
            printf("FAILED: %s u=%u wrote outside its 65536 bytes\n", what, u);
            free(buf);
            return 1;
        }
    for (int b = 0; b < 256; b++)
        for (int v = 0; v < 256; v++) {
            const unsigned long r = (2ul * q[b][v] + u) / (2ul * u);
            const unsigned want = v == 255 ? 255u : (r < 254ul ? (unsigned)r : 254u);

            if (t[b][v] != want) {
                printf("FAILED: %s u=%u t[%d][%d] = %u, want %u\n", what, u, b, v, (unsigned)t[b][v], want);
                free(buf);
                return 1;
            }
        }
    free(buf);
    return 0;
}

int main(int argc, char **argv)
{
    static const unsigned units[] = { 1, 13, 100, 250, 65000 };
    static const double rain_units[] = { 1.0, 2.5, 0.37, 2.54 };
    static const char *const bad[] = { "", " 1", "1 ", "x", "1,2", "0", "0.0049", "-1", "650.01", "nan", "inf", "1mm",
                                       "1e999", "-", "+", ".", "1e", ",", NULL };
    static const struct { const char *text; unsigned u; } good[] = { { "1", 100 }, { "2.5", 250 }, { "0.01", 1 },
                                                                     { "650", 65000 }, { ".5", 50 }, { "0.125", 13 } };
    uint16_t (*q)[256] = malloc(256 * sizeof *q);
    unsigned u = 77;

    if (argc == 2) {
        free(q);
        if (gcn10_parse_runoff_unit(argv[1], &u) != 0) {
            printf("bad\n");
            return 1;
        }
        printf("%u\n", u);
        return 0;
    }
    if (!q)
        return 1;
    for (size_t i = 0; i < sizeof units / sizeof units[0]; i++) {
        for (int b = 0; b < 256; b++)
            for (int v = 0; v < 256; v++)
                q[b][v] = (uint16_t)rnd();
        q[0][0] = 65535;
        q[0][1] = 0;
        if (check_tables(q, units[i], "random tables") != 0)
            return 1;
        gcn10_rain_tables(2.5, 0.2, q);
        if (check_tables(q, units[i], "rain tables") != 0)
            return 1;
    }
    for (size_t i = 0; i < sizeof rain_units / sizeof rain_units[0]; i++) {
        uint8_t (*t)[256] = malloc(256 * sizeof *t);

        if (!t)
            return 1;
        gcn10_rain_tables(rain_units[i], 0.2, q);
        u = gcn10_runoff_unit_of(rain_units[i]);
        gcn10_runoff_bytes(q, u, t);
        for (int b = 0; b < 255; b++)
            for (int v = 0; v < 255; v++)
                if (t[b][v] > b) {
                    printf("FAILED: unit %g: t[%d][%d] = %u is more than the rain\n", rain_units[i], b, v, (unsigned)t[b][v]);
                    return 1;
                }
        free(t);
    }
    if (gcn10_parse_runoff_unit(NULL, &u) == 0 || gcn10_runoff_unit_of(0.0) != 1 || gcn10_runoff_unit_of(1e9) != 65000) {
        printf("FAILED: a null text, or the clamps of the default unit\n");
        return 1;
    }
    for (int i = 0; bad[i]; i++) {
        u = 77;
        if (gcn10_parse_runoff_unit(bad[i], &u) == 0 || u != 77) {
            printf("FAILED: '%s' is taken, or *u is written\n", bad[i]);
            return 1;
        }
    }
    for (size_t i = 0; i < sizeof good / sizeof good[0]; i++)
        if (gcn10_parse_runoff_unit(good[i].text, &u) != 0 || u != good[i].u) {
            printf("FAILED: '%s' gives %u, want %u\n", good[i].text, u, good[i].u);
            return 1;
        }
    free(q);
    printf("cases ok\n");
    return 0;
}
