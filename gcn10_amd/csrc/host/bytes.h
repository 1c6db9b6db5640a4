/* bytes.h -- integers and doubles as they lie in TIFF, shapefile and dBase files, whatever the host's byte order. */
#ifndef GCN10_BYTES_H
#define GCN10_BYTES_H

#include <stdbool.h>
#include <stdint.h>
#include <string.h>

/* n bytes in the file's order: little endian, or big endian when `swap` */
static inline uint64_t rd(const unsigned char *p, int n, bool swap)
{
    uint64_t v = 0;

    if (swap)
        for (int i = 0; i < n; i++)
            v = (v << 8) | p[i];
    else
        for (int i = n - 1; i >= 0; i--)
            v = (v << 8) | p[i];
    return v;
}

static inline uint32_t be32(const unsigned char *p)
{
    return (uint32_t)rd(p, 4, true);
}

static inline uint32_t le32(const unsigned char *p)
{
    return (uint32_t)rd(p, 4, false);
}

static inline double le_f64(const unsigned char *p)
{
    uint64_t v = rd(p, 8, false);
    double d;

    memcpy(&d, &v, sizeof d);
    return d;
}

static inline void put16(unsigned char *p, unsigned v)
{
    p[0] = (unsigned char)(v & 0xff);
    p[1] = (unsigned char)(v >> 8);
}

static inline void put32(unsigned char *p, uint32_t v)
{
    put16(p, v & 0xffff);
    put16(p + 2, v >> 16);
}

#endif
