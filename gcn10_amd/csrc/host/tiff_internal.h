/* tiff_internal.h -- what the files of the GeoTIFF module share.
 *
 * The module replaces what the reference gets from GDAL in load_raster() / save_raster() (src/raster.c:106-227) for
 * the file kinds this program meets, without GDAL or libtiff:
 *   read : 8-bit single-band (or pixel-interleaved, band 1 taken) TIFF, classic or BigTIFF, either byte order,
 *          strips or tiles, compression none / LZW (5) / Adobe DEFLATE (8, 32946) / PackBits (32773), predictor
 *          1|2, georeferenced by ModelPixelScale + ModelTiepoint or ModelTransformation, any directory of the
 *          file's chain (the overviews of a Cloud Optimized GeoTIFF);
 *   write: classic little-endian GTiff, Byte, 1 band, 256 x 256 tiles that arrive compressed (Adobe DEFLATE, the
 *          creation options of src/raster.c:204-209, or LZW), as a plain file -- tile data, then the directory -- or
 *          as a Cloud Optimized GeoTIFF -- ghost area, every directory, then the overviews' tiles and the raster's --
 *          with the input's GeoKey tags copied so the projection is the landcover's (src/raster.c:212-214), and
 *          GDAL_NODATA / GDAL_METADATA tags where the run asks for them.
 * The files:
 *   tiff_open.c    header, directory walk, tags, chunk layout, geotransform; the accessors of an open file
 *   tiff_codec.c   one chunk from file bytes to pixels: LZW, PackBits, zlib, predictor 2
 *   tiff_cache.c   decoded chunks kept for the windows that use a small part of them
 *   tiff_window.c  a window of pixels (host reader) and the plan of its chunks (GPU decoders)
 *   tiff_write.c   the tiled writer
 * Format sources: TIFF 6.0 (1992), BigTIFF design note, GeoTIFF 1.0 / OGC 19-008r4, GDAL's COG driver notes.
 * File *bytes* are not a parity target (GDAL's encoder is third party); decoded pixels and geotransform are.
 */
#ifndef GCN10_TIFF_INTERNAL_H
#define GCN10_TIFF_INTERNAL_H

#include "host_internal.h"
#include "bytes.h"

enum { T_BYTE = 1, T_ASCII = 2, T_SHORT = 3, T_LONG = 4, T_RATIONAL = 5, T_SBYTE = 6,
       T_UNDEF = 7, T_SSHORT = 8, T_SLONG = 9, T_SRATIONAL = 10, T_FLOAT = 11,
       T_DOUBLE = 12, T_IFD = 13, T_LONG8 = 16, T_SLONG8 = 17, T_IFD8 = 18 };

struct gcn10_tiff {
    int fd;
    bool big, swap;
    uint32_t width, height;
    uint16_t bps, spp, compression, predictor, planar;
    bool tiled;
    uint32_t cw, ch;            /* chunk (tile or strip) width / height */
    uint32_t across, down;      /* chunks per row / column */
    uint64_t *offsets, *counts;
    uint64_t n_chunks;
    uint64_t file_size;
    uint64_t id_dev, id_ino;    /* which file (the chunk cache is shared by every open handle of it) */
    uint64_t next_ifd;          /* offset of the directory behind the one that was read, 0 = none */
    uint16_t spp_file;          /* SamplesPerPixel as the file says (spp is 1 for band-sequential files) */
    double gt[6];
    gcn10_georef georef;
};

/* tiff_open.c: n bytes at a file position, all of them; 0 or -1 */
int gcn10_pread_all(int fd, void *buf, size_t n, uint64_t off);
/* whether the bytes the directory names for chunk idx lie inside the file (a chunk of 0 bytes at a position in it does) */
bool gcn10_tiff_chunk_in_file(const struct gcn10_tiff *t, uint64_t idx);

/* tiff_codec.c: the first `need` bytes of chunk `idx` into buf (the chunk holds cw * rows_in_chunk * spp bytes; a
 * chunk of 0 bytes reads as zeros); *scratch grows to hold the compressed bytes.  0 or -1. */
int gcn10_tiff_decode_chunk(struct gcn10_tiff *t, uint64_t idx, unsigned char *buf, size_t rawcap,
                            unsigned char **scratch, size_t *scratch_cap, uint32_t rows_in_chunk, size_t need);

/* tiff_cache.c: the process-wide cache of decoded chunks */
struct gcn10_cache_entry {
    uint64_t dev, ino, idx;
    unsigned char *data;
    size_t bytes;
    uint64_t stamp;
    int refs;
};
bool gcn10_chunk_cache_enabled(void);
/* the chunk's decoded bytes (pinned until released), or NULL */
struct gcn10_cache_entry *gcn10_chunk_cache_get(const struct gcn10_tiff *t, uint64_t idx, size_t bytes);
/* hands `data` (malloc'ed, `bytes` long) to the cache; returns the entry to read from (pinned), or NULL when the cache
 * does not take it (the caller keeps and frees `data`) */
struct gcn10_cache_entry *gcn10_chunk_cache_put(const struct gcn10_tiff *t, uint64_t idx, unsigned char *data,
                                                size_t bytes);
void gcn10_chunk_cache_release(struct gcn10_cache_entry *c);

#endif
