/* runoff.c -- the design storm of the runoff-weighted composites (config key "storm", --storm), and a ladder of them
 * (config key "storms", --storms): no counterpart in the reference.
 *
 * A storm is a rainfall depth P in mm and an initial-abstraction ratio lambda.  The SCS runoff depth of a curve number
 * is a table of 256 16-bit values in units of 0.01 mm, made here in plain IEEE double (this file is built with
 * -ffp-contract=off, as geo.c is) in the operation order stated in include/gcn10_host.h; everything after the table is
 * integers: a cell's or a zone's sum of table values, and the smallest curve number whose runoff over the whole cell
 * reaches that sum.
 *
 * A rainfall raster (config keys "rain" / "rain_unit") is 256 such storms, one per count of the raster's byte: the unit
 * parser and the 256 tables are here, the raster itself is read by grid.c (gcn10_rain_load).  Several of them in one run
 * (config key "rains") share the unit and the tables: the parser of the file list and the bytes of a cell from its 2 + K
 * words are here too.
 *
 * Per-pixel runoff rasters (config key "runoff_rain"): the 256 tables as bytes in an output unit, and the parser of that
 * unit, are here; the run mode is runoff_raster.c.
 */
#include "gcn10_host.h"

#include <errno.h>
#include <math.h>
#include <stdbool.h>
#include <stdlib.h>
#include <string.h>

#if defined(__GNUC__) && !defined(__clang__)
#define NO_CONTRACT __attribute__((optimize("fp-contract=off")))
#else
#define NO_CONTRACT
#pragma STDC FP_CONTRACT OFF
#endif

int gcn10_parse_storm(const char *text, double *P, double *lambda)
{
    double d[2] = { 0.0, 0.2 };
    const char *p = text;
    char *end;

    if (!text)
        return -1;
    for (int i = 0; i < 2; i++) {
        /* strtod skips leading white space and takes "inf" and "nan": a field starts with a sign, a digit or a point,
         * and the values are checked below */
        if (!(*p == '-' || *p == '+' || *p == '.' || (*p >= '0' && *p <= '9')))
            return -1;
        errno = 0;
        d[i] = strtod(p, &end);
        if (end == p || errno != 0 || (*end != '\0' && !(i == 0 && *end == ',')))
            return -1;
        if (*end == '\0')
            break;
        p = end + 1;
    }
    if (!isfinite(d[0]) || !isfinite(d[1]) || !(d[0] > 0.0) || !(d[0] <= 650.0) || !(d[1] >= 0.0) || !(d[1] < 1.0))
        return -1;
    *P = d[0];
    *lambda = d[1];
    return 0;
}

int gcn10_parse_storms(const char *text, double P[GCN10_MAX_STORMS], int *k, double *lambda)
{
    double d[GCN10_MAX_STORMS], lam = 0.2;
    uint16_t q[256];
    const char *p = text;
    char *end;
    int n = 0;
    unsigned last = 0;

    if (!text)
        return -1;
    for (bool ratio = false;;) {
        double v;

        /* a field as gcn10_parse_storm takes it: a sign, a digit or a point first, nothing but the number */
        if (!(*p == '-' || *p == '+' || *p == '.' || (*p >= '0' && *p <= '9')))
            return -1;
        errno = 0;
        v = strtod(p, &end);
        if (end == p || errno != 0 || !isfinite(v))
            return -1;
        if (ratio) {
            if (*end != '\0' || !(v >= 0.0) || !(v < 1.0))
                return -1;
            lam = v;
            break;
        }
        if (n == GCN10_MAX_STORMS || !(v > 0.0) || !(v <= 650.0))
            return -1;
        d[n++] = v;
        if (*end == '\0')
            break;
        if (*end == ',')
            ratio = true;
        else if (*end != ':')
            return -1;
        p = end + 1;
    }
    for (int i = 0; i < n; i++) {           /* rising in the unit of the names */
        gcn10_runoff_table(d[i], lam, q);
        if (i > 0 && q[100] <= last)
            return -1;
        last = q[100];
    }
    for (int i = 0; i < n; i++)
        P[i] = d[i];
    *k = n;
    *lambda = lam;
    return 0;
}

int gcn10_parse_rain_unit(const char *text, double *unit, double *lambda)
{
    double d[2] = { 1.0, 0.2 };
    const char *p = text;
    char *end;

    if (!text)
        return -1;
    for (int i = 0; i < 2; i++) {
        /* a field as gcn10_parse_storm takes it: a sign, a digit or a point first, nothing but the number */
        if (!(*p == '-' || *p == '+' || *p == '.' || (*p >= '0' && *p <= '9')))
            return -1;
        errno = 0;
        d[i] = strtod(p, &end);
        if (end == p || errno != 0 || (*end != '\0' && !(i == 0 && *end == ',')))
            return -1;
        if (*end == '\0')
            break;
        p = end + 1;
    }
    if (!isfinite(d[0]) || !isfinite(d[1]) || !(d[0] > 0.0) || !(255.0 * d[0] <= 650.0) || !(d[1] >= 0.0) ||
        !(d[1] < 1.0))
        return -1;
    *unit = d[0];
    *lambda = d[1];
    return 0;
}

int gcn10_parse_rains(const char *text, char **copy, const char *files[GCN10_MAX_RAINS], int *k)
{
    size_t len, members = 1;
    char *c;
    int n = 0;

    if (!text || !*text)
        return -1;
    len = strlen(text);
    for (size_t i = 0; i < len; i++) {
        const bool first = i == 0 || text[i - 1] == ':';

        if (text[i] == ':' && (first || i + 1 == len))      /* an empty member, the last one included */
            return -1;
        members += text[i] == ':';
    }
    if (members > GCN10_MAX_RAINS || !(c = malloc(len + 1)))
        return -1;
    memcpy(c, text, len + 1);
    for (size_t i = 0; i < len; i++) {
        if (i == 0 || text[i - 1] == ':')
            files[n++] = c + i;
        if (c[i] == ':')
            c[i] = '\0';
    }
    *copy = c;
    *k = n;
    return 0;
}

void gcn10_rains_cell(const uint64_t *words, int k, const uint8_t bytes[], const uint16_t q[256][256], uint8_t cn[])
{
    for (int j = 0; j < k; j++)
        cn[j] = (uint8_t)gcn10_runoff_cn(words[0], words[1], words[2 + j], q[bytes[j]]);
}

NO_CONTRACT void gcn10_rain_tables(double unit, double lambda, uint16_t q[256][256])
{
    for (int b = 0; b < 256; b++)
        gcn10_runoff_table((double)b * unit, lambda, q[b]);
}

NO_CONTRACT void gcn10_runoff_table(double P, double lambda, uint16_t q[256])
{
    q[0] = q[255] = 0;
    for (int v = 1; v < 255; v++) {
        const double c = v < 100 ? (double)v : 100.0;
        const double S = 25400.0 / c - 254.0;
        const double Ia = lambda * S;

        if (!(P > Ia)) {
            q[v] = 0;
        }
        else {
            const double e = P - Ia;
            const double r = floor(e * e / (e + S) * 100.0 + 0.5);

            q[v] = (uint16_t)(r < 0.0 ? 0.0 : (r > 65535.0 ? 65535.0 : r));     /* 0 < P <= 650: r <= 65000 */
        }
    }
}

int gcn10_runoff_cn(uint64_t s, uint64_t n, uint64_t sw, const uint16_t q[256])
{
    if (n == 0)
        return 255;                         /* no value, as in every raster */
    if (sw == 0)
        return (int)((2 * s + n) / (2 * n));
    for (int c = 1; c < 100; c++)
        if (n * (uint64_t)q[c] >= sw)
            return c;
    return 100;
}

NO_CONTRACT int gcn10_zone_rain_values(uint64_t rain_pixels, uint64_t rain_sum, double unit, double lambda, uint64_t s,
                                       uint64_t n, uint64_t sw, double *rain_mm, double *runoff_mm, int *cn)
{
    uint16_t q[256];

    *rain_mm = *runoff_mm = 0.0;
    *cn = 255;
    if (rain_pixels == 0)
        return 0;
    *rain_mm = ((double)rain_sum / (double)rain_pixels) * unit;
    if (n == 0)
        return 1;
    *runoff_mm = (double)sw / (double)n / 100.0;
    gcn10_runoff_table(*rain_mm, lambda, q);
    *cn = gcn10_runoff_cn(s, n, sw, q);
    return 3;
}

void gcn10_runoff_bytes(const uint16_t q[256][256], unsigned u, uint8_t t[256][256])
{
    for (int b = 0; b < 256; b++) {
        for (int v = 0; v < 255; v++) {
            const unsigned r = (2u * (unsigned)q[b][v] + u) / (2u * u);

            t[b][v] = (uint8_t)(r < 254u ? r : 254u);
        }
        t[b][255] = 255;
    }
}

NO_CONTRACT unsigned gcn10_runoff_unit_of(double mm)
{
    const double r = floor(100.0 * mm + 0.5);

    return !(r >= 1.0) ? 1u : (r > 65000.0 ? 65000u : (unsigned)r);
}

NO_CONTRACT int gcn10_parse_runoff_unit(const char *text, unsigned *u)
{
    char *end;
    double x, r;

    if (!text)
        return -1;
    /* a field as gcn10_parse_storm takes it: a sign, a digit or a point first, nothing but the number */
    if (!(*text == '-' || *text == '+' || *text == '.' || (*text >= '0' && *text <= '9')))
        return -1;
    errno = 0;
    x = strtod(text, &end);
    if (end == text || errno != 0 || *end != '\0' || !isfinite(x))
        return -1;
    r = floor(100.0 * x + 0.5);
    if (!(r >= 1.0) || !(r <= 65000.0))
        return -1;
    *u = (unsigned)r;
    return 0;
}
