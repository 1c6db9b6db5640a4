/* tiff_codec.c -- one chunk (tile or strip) from the bytes in the file to pixels, on the host: TIFF LZW, PackBits,
 * zlib for DEFLATE, and the undo of predictor 2.  (The module as a whole: tiff_internal.h.)
 */
#include "tiff_internal.h"

#include <stdlib.h>
#include <string.h>
#include <zlib.h>

/* TIFF LZW (TIFF 6.0 section 13): MSB-first codes of 9..12 bits, ClearCode 256,
 * EndOfInformation 257, "early change" of the code width. */
static int lzw_decode(const unsigned char *src, size_t n, unsigned char *dst, size_t cap)
{
    enum { CLEAR = 256, EOI = 257, FIRST = 258, MAXC = 4096 };
    static __thread uint16_t prefix[MAXC];
    static __thread unsigned char suffix[MAXC], first[MAXC];
    static __thread uint16_t length[MAXC];
    uint32_t bits = 0;
    int nbits = 0, width = 9, next = FIRST, prev = -1;
    size_t ip = 0, op = 0;

    for (int i = 0; i < 256; i++) {
        prefix[i] = 0;
        suffix[i] = first[i] = (unsigned char)i;
        length[i] = 1;
    }
    for (;;) {
        int code;

        while (nbits < width) {
            if (ip >= n)
                return op == cap ? 0 : -1;      /* stream ended without EOI */
            bits = (bits << 8) | src[ip++];
            nbits += 8;
        }
        code = (int)((bits >> (nbits - width)) & ((1u << width) - 1));
        nbits -= width;
        if (code == EOI) {
            if (op < cap)               /* an early EOI leaves zeros, as a short DEFLATE chunk does */
                memset(dst + op, 0, cap - op);
            break;
        }
        if (code == CLEAR) {
            width = 9;
            next = FIRST;
            prev = -1;
            continue;
        }
        if (prev < 0) {
            if (code >= 256 || op >= cap)
                return op >= cap ? 0 : -1;
            dst[op++] = (unsigned char)code;
            prev = code;
            if (op >= cap)
                return 0;               /* chunk complete; trailing codes are padding */
            continue;
        }
        {
            /* the string of `code`; code == next is the KwKwK case: string(prev) + its
             * own first byte */
            const bool kwkwk = code == next;
            size_t full, pos;
            unsigned char fc;
            int c;

            if (code > next || (kwkwk && next >= MAXC))
                return -1;
            fc = kwkwk ? first[prev] : first[code];
            full = kwkwk ? (size_t)length[prev] + 1 : (size_t)length[code];
            pos = full;
            c = kwkwk ? prev : code;
            if (kwkwk) {
                pos--;
                if (op + pos < cap)
                    dst[op + pos] = fc;
            }
            while (pos > 0) {           /* strings are stored as (prefix, last byte) */
                pos--;
                if (op + pos < cap)
                    dst[op + pos] = suffix[c];
                c = prefix[c];
            }
            op += full;
            if (next < MAXC) {
                prefix[next] = (uint16_t)prev;
                suffix[next] = fc;
                first[next] = first[prev];
                length[next] = (uint16_t)(length[prev] + 1);
                next++;
                if (next + 1 >= (1 << width) && width < 12)    /* early change */
                    width++;
            }
            prev = code;
            if (op >= cap)
                return 0;               /* chunk complete; trailing codes are padding */
        }
    }
    return 0;
}

static int packbits_decode(const unsigned char *src, size_t n, unsigned char *dst, size_t cap)
{
    size_t ip = 0, op = 0;

    while (ip < n && op < cap) {
        int c = (signed char)src[ip++];

        if (c >= 0) {
            size_t len = (size_t)c + 1;

            if (ip + len > n)
                return -1;
            if (op + len > cap)
                len = cap - op;
            memcpy(dst + op, src + ip, len);
            ip += (size_t)c + 1;
            op += len;
        }
        else if (c != -128) {
            size_t len = (size_t)(1 - c);

            if (ip >= n)
                return -1;
            if (op + len > cap)
                len = cap - op;
            memset(dst + op, src[ip++], len);
            op += len;
        }
    }
    return 0;
}

/* horizontal differencing undone, per row, per sample, over the first `want` bytes of a chunk */
static void undo_predictor2(const struct gcn10_tiff *t, unsigned char *buf, uint32_t rows_in_chunk, size_t want)
{
    const size_t rowb = (size_t)t->cw * t->spp;

    for (uint32_t r = 0; r < rows_in_chunk && (size_t)r * rowb < want; r++) {
        unsigned char *row = buf + (size_t)r * rowb;
        size_t end = want - (size_t)r * rowb < rowb ? want - (size_t)r * rowb : rowb;

        for (size_t i = t->spp; i < end; i++)
            row[i] = (unsigned char)(row[i] + row[i - t->spp]);
    }
}

/* A window that ends early in a chunk -- a few columns of a full-width strip, as in the soil raster -- does not pay
 * for the rest of it: only the first `need` bytes are decoded.  (The Predictor tag belongs to the LZW / DEFLATE /
 * PackBits codecs: libtiff, and with it GDAL, ignores it on uncompressed data, and so does this.) */
int gcn10_tiff_decode_chunk(struct gcn10_tiff *t, uint64_t idx, unsigned char *buf, size_t rawcap,
                            unsigned char **scratch, size_t *scratch_cap, uint32_t rows_in_chunk, size_t need)
{
    uint64_t off = t->offsets[idx], cnt = t->counts[idx];
    size_t want = (size_t)t->cw * rows_in_chunk * t->spp;

    if (want > rawcap)
        return -1;
    if (need < want)
        want = need;
    if (!gcn10_tiff_chunk_in_file(t, idx))
        return -1;                  /* chunk outside the file: corrupt directory */
    if (cnt == 0) {                 /* sparse tile: GDAL reads it as zeros */
        memset(buf, 0, want);
        return 0;
    }
    if (t->compression == 1) {
        if (cnt < want)
            return -1;
        return gcn10_pread_all(t->fd, buf, want, off);
    }
    if (cnt > *scratch_cap) {
        unsigned char *g = realloc(*scratch, (size_t)cnt);

        if (!g)
            return -1;
        *scratch = g;
        *scratch_cap = (size_t)cnt;
    }
    if (gcn10_pread_all(t->fd, *scratch, (size_t)cnt, off) != 0)
        return -1;
    if (t->compression == 8 || t->compression == 32946) {
        uLongf dl = (uLongf)want;
        int rc = uncompress(buf, &dl, *scratch, (uLong)cnt);

        /* Z_BUF_ERROR with a full buffer = stream longer than the chunk (padding) */
        if (rc != Z_OK && !(rc == Z_BUF_ERROR && dl == want))
            return -1;
        if (dl < want)
            memset(buf + dl, 0, want - dl);
    }
    else if (t->compression == 5) {
        if (lzw_decode(*scratch, (size_t)cnt, buf, want) != 0)
            return -1;
    }
    else {
        if (packbits_decode(*scratch, (size_t)cnt, buf, want) != 0)
            return -1;
    }
    if (t->predictor == 2)
        undo_predictor2(t, buf, rows_in_chunk, want);
    return 0;
}
