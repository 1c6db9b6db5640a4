/* stats.c -- band statistics of the CN rasters (config keys "stats" and "nodata").
 *
 * GDAL computes a band's statistics on first use by reading the whole raster unless the file carries them in its
 * GDAL_METADATA tag.  The GPU counts one histogram per block over (landcover, soil code) pairs
 * (gcn10_gpu_pair_histogram); every raster's value is a function of that pair, so each raster's exact histogram,
 * and from it the statistics, follow here on the host.  The numbers are formed the way GDAL's
 * GDALRasterBand::ComputeStatistics forms them for a Byte band (exact integer sums; the standard deviation from
 * n * sum(v^2) - sum(v)^2 in 128-bit integers) and printed as SetStatistics prints them ("%.14g"; the valid
 * percent "%.4g").  GDAL is not used here, so this formatting is pinned by tests/test_stats_host.py.
 */
#include "gcn10_host.h"
#include "host_internal.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

/* the value of a (landcover, soil plane) pair: src/cn.c:114-131 with the 255 pre-fill of src/cn.c:289: only values
 * < 255 are stored, as (uint8_t) */
static inline int pair_value(const int table[256][5], int lc, int plane)
{
    return plane < 5 && table[lc][plane] < 255 ? (uint8_t)table[lc][plane] : 255;
}

void gcn10_raster_histogram(const uint64_t *pair, const uint8_t codes[16], const int table[256][5], int drained,
                            uint64_t hist[256])
{
    memset(hist, 0, 256 * sizeof *hist);
    for (int b = 0; b < 16; b++) {
        const int plane = drained ? (codes[b] & 15) : (codes[b] >> 4);

        for (int lc = 0; lc < 256; lc++) {
            const uint64_t n = pair[b * 256 + lc];

            if (n)
                hist[pair_value(table, lc, plane)] += n;
        }
    }
}

void gcn10_raster_histogram_sparse(const uint16_t *at, const uint64_t *n, size_t m, const uint8_t codes[16],
                                   const int table[256][5], int drained, uint64_t hist[256])
{
    memset(hist, 0, 256 * sizeof *hist);
    for (size_t i = 0; i < m; i++) {
        const int b = at[i] >> 8, plane = drained ? (codes[b] & 15) : (codes[b] >> 4);

        hist[pair_value(table, at[i] & 255, plane)] += n[i];
    }
}

void gcn10_band_stats_of(const uint64_t hist[256], int nodata, gcn10_band_stats *st)
{
    uint64_t sum = 0;
    unsigned __int128 sum2 = 0, var;

    memset(st, 0, sizeof *st);
    st->min = 255;
    st->max = 0;
    for (int v = 0; v < 256; v++) {
        st->total += hist[v];
        if (!hist[v] || v == nodata)
            continue;
        st->valid += hist[v];
        sum += hist[v] * (uint64_t)v;                       /* < 2^64: at most 255 * 2^56 pixels */
        sum2 += (unsigned __int128)hist[v] * (uint64_t)(v * v);
        if (v < st->min)
            st->min = v;
        if (v > st->max)
            st->max = v;
    }
    if (!st->valid) {
        st->min = st->max = 0;
        return;
    }
    st->mean = (double)sum / (double)st->valid;
    var = sum2 * st->valid - (unsigned __int128)sum * sum;  /* n^2 * population variance, exact */
    st->stddev = sqrt((double)var) / (double)st->valid;
    st->valid_percent = 100.0 * (double)st->valid / (double)st->total;
}

size_t gcn10_stats_xml(const gcn10_band_stats *st, char *buf, size_t cap)
{
    int n;

    if (!st->valid)
        return 0;
    n = snprintf(buf, cap,
                 "<GDALMetadata>\n"
                 "  <Item name=\"STATISTICS_MAXIMUM\" sample=\"0\">%.14g</Item>\n"
                 "  <Item name=\"STATISTICS_MEAN\" sample=\"0\">%.14g</Item>\n"
                 "  <Item name=\"STATISTICS_MINIMUM\" sample=\"0\">%.14g</Item>\n"
                 "  <Item name=\"STATISTICS_STDDEV\" sample=\"0\">%.14g</Item>\n"
                 "  <Item name=\"STATISTICS_VALID_PERCENT\" sample=\"0\">%.4g</Item>\n"
                 "</GDALMetadata>\n",
                 (double)st->max, st->mean, (double)st->min, st->stddev, st->valid_percent);
    return n > 0 && (size_t)n < cap ? (size_t)n : 0;
}
