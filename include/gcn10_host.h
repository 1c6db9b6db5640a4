/*
 * gcn10_host.h -- host side (plain C99) of the MI355X curve-number generator.
 *
 * These are the pieces of gcn10's src/ program that stay on the CPU: the
 * lookup-CSV loader, the fp64 geotransform arithmetic that must be bit-exact,
 * config / logging / block list handling, raster I/O and the per-GPU block
 * queue that drives include/gcn10_gpu.h.  Every declaration names the
 * reference code whose behaviour it keeps (paths under /root/reference).
 */
#ifndef GCN10_HOST_H
#define GCN10_HOST_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCN10_VERSION "0.1.0"          /* src/main.c:12-14 */

/* ------------------------------------------------------------------------ */
/* lookup tables (src/cn.c:13-85)                                           */
/* ------------------------------------------------------------------------ */

/* hydrologic conditions and ARCs in the reference's loop order
 * (src/cn.c:146-147); table k = hc*3 + arc. */
extern const char *const gcn10_hcs[3];      /* "p", "f", "g"     */
extern const char *const gcn10_arcs[3];     /* "i", "ii", "iii"  */
extern const char *const gcn10_conds[2];    /* "drained", "undrained" (src/cn.c:145) */

/* Callback for the rows load_lookup_table() logs as ERROR and skips
 * (src/cn.c:58-63, 68-73, 78-82).  May be NULL. */
typedef void (*gcn10_row_error_fn)(void *user, const char *message);

/* Parses one lookup CSV into the reference's int table[256][5].
 * Returns 0, -1 when the file cannot be opened (src/cn.c:28-33) and -2 when it
 * is empty (src/cn.c:43-48); the reference aborts the run in both cases and so
 * does the gcn10 program. */
int gcn10_load_lookup_file(const char *path, int table[256][5],
                           gcn10_row_error_fn on_error, void *user);

/* "<dir>/default_lookup_<hc>_<arc>.csv" (src/cn.c:21).  -3: path too long. */
int gcn10_load_lookup_table(const char *dir, const char *hc, const char *arc,
                            int table[256][5], gcn10_row_error_fn on_error,
                            void *user);

/* All nine tables in k = hc*3+arc order; stops at the first failure and
 * returns its code (failed_k, if not NULL, receives the table index). */
int gcn10_load_all_lookup_tables(const char *dir, int tables[9][256][5],
                                 int *failed_k, gcn10_row_error_fn on_error,
                                 void *user);

/* ------------------------------------------------------------------------ */
/* geotransform arithmetic                                                   */
/* ------------------------------------------------------------------------ */

/* The separable index maps of the resample loop, src/cn.c:218-229:
 *   ci[x] = clamp((int)round((gt[0]+(x+0.5)*gt[1] - soil_gt[0]) / soil_gt[1]), 0, hsx-1)
 *   cj[y] = clamp((int)round((soil_gt[3] - (gt[3]+(y+0.5)*gt[5])) / fabs(soil_gt[5])), 0, hsy-1)
 * evaluated in IEEE double, in the reference's operation order, without
 * fused multiply-add (this file is built with -ffp-contract=off), and with the
 * reference build's x86-64 double->int conversion. */
void gcn10_build_index_maps(const double gt[6], const double soil_gt[6],
                            int W, int H, int hsx, int hsy,
                            int32_t *ci, int32_t *cj);

/* Window of a raster (geotransform t, size rx x ry) covering bbox
 * {minx, miny, maxx, maxy}: src/raster.c:126-162.  Returns 0, or -1 for the
 * "invalid raster bounds" case (src/raster.c:142-147). */
int gcn10_raster_window(const double t[6], int rx, int ry, const double bbox[4],
                        int *xoff, int *yoff, int *xcount, int *ycount,
                        double gt[6]);


/* ------------------------------------------------------------------------ */
/* config (src/config.c) and logging (src/log.c)                            */
/* ------------------------------------------------------------------------ */

/* The five required keys of the reference's config file (src/config.c:69-103,
 * 107-113) plus optional keys this program adds; unknown keys and lines
 * without '=' are ignored, '#' starts a comment line, lines are cut at 511
 * bytes (src/config.c:47-64). */
#define GCN10_MAX_STORMS 8      /* design storms of one run (config key "storms") */

typedef struct gcn10_config {
    char *hysogs_data_path;
    char *esa_data_path;
    char *blocks_shp_path;
    char *lookup_table_path;
    char *log_dir;
    /* optional extensions (absent = default) */
    int gpus;               /* "gpus": number of GPUs to use, 0 = all visible      */
    int workers_per_gpu;    /* "workers_per_gpu": block workers per GPU, 0 = default 2 */
    int strip_rows;         /* "strip_rows": rows per staging strip, rounded up to whole tile rows; 0 = default 2304 */
    int io_threads;         /* "io_threads": tile compression threads, 0 = auto    */
    int deflate_level;      /* "deflate_level": zlib level 1..9, 0 = zlib default 6 */
    char *esa_tile_dir;     /* "esa_tile_dir": local mirror of /vsicurl/ VRT sources */
    int gpu_deflate;        /* "gpu_deflate": 2 (default) fused: tiles are DEFLATE-encoded on the
                               GPU straight from landcover + soil, no CN raster in HBM;
                               1 = CN strips in HBM, then encoded on the GPU per raster;
                               0 = raw strips are copied back, host zlib threads encode */
    int gpu_inflate;        /* "gpu_inflate": 1 (default) DEFLATE-compressed landcover tiles cross PCIe
                               compressed and are decoded on the GPU, uncompressed ones are untiled there,
                               TIFF predictor 2 is undone there; 0 = all of it on the host i/o pool */
    int direct_io;          /* "direct_io": 1 = the GeoTIFFs' tile data is written with O_DIRECT from the pinned
                               copy of the encoder's arena (no page-cache copy); 0 (default) = buffered writes */
    int prefetch_blocks;    /* "prefetch_blocks": 1 (default) = every block worker has an input thread that stages
                               and decodes the NEXT block's landcover while this one is encoded; 0 = in turn */
    unsigned table_mask;    /* "lookups": which of the nine lookups to produce, e.g. "g_ii" or "p_i,f_iii"
                               ("all" / absent = all nine); bit k = hc*3 + arc in the reference's loop
                               order p,f,g x i,ii,iii (src/cn.c:146-147) */
    unsigned cond_mask;     /* "conditions": "drained", "undrained" or "both" (absent = both);
                               bit 0 = drained, bit 1 = undrained (src/cn.c:145) */
    int compress;           /* "compress": GCN10_COMPRESS_DEFLATE (default, "deflate") or GCN10_COMPRESS_LZW ("lzw"),
                               case-insensitive as GDAL's COMPRESS=; LZW tiles are encoded on the GPU only, so
                               "lzw" with gpu_deflate=0 is refused */
    int gpu_inflate_lzw;    /* "gpu_inflate_lzw": 1 (default) with gpu_inflate=1, LZW-compressed landcover tiles
                               cross PCIe compressed and are decoded on the GPU too (when the GPU library has the
                               decoder: gcn10_gpu_inflate_codecs); 0 = LZW windows through the host reader */
    int cog;                /* "cog": 1 = Cloud Optimized GeoTIFFs with overviews (gcn10_tiff_create_cog), built on the
                               GPU; 0 (default) = plain tiled GeoTIFFs.  No host fallback: refused with gpu_deflate=0 */
    int overview_resampling;/* "overview_resampling": GCN10_OVERVIEW_NEAREST (default, "nearest") or
                               GCN10_OVERVIEW_AVERAGE ("average"), any case */
    int stats;              /* "stats": 1 = every written raster carries GDAL band statistics (STATISTICS_* items in
                               its GDAL_METADATA tag, 42112), counted on the GPU; 0 (default) = none */
    int nodata;             /* "nodata": 0..255 = every written raster declares that NoData value (GDAL_NODATA tag,
                               42113) and its statistics leave it out; -1 ("none", default) = no tag */
    int verify;             /* "verify": 1 = nothing is written: the rasters that exist are decoded on the GPU and every
                               pixel is compared with the value computed now (gcn10_verify_*); 0 (default) = a write run */
    int zonal;              /* "zonal": 1 = nothing is written but one table: the composite (mean) curve number of every
                               zone of zones_shp_path and every selected raster, counted on the GPU (zonal.c); 0 (default) */
    char *zones_shp_path;   /* "zones_shp_path": polygon shapefile of the zones, in the landcover's CRS (needed by zonal=1) */
    char *zones_id_field;   /* "zones_id_field": numeric .dbf field that names a zone (absent = "ID") */
    char *zonal_output;     /* "zonal_output": the table's path, relative to the CWD as the rasters are (absent = zonal_cn.csv) */
    int aggregate;          /* "aggregate": f = 2..256: no 10 m raster is written but the area mean of every selected raster
                               over cells of f x f landcover pixels, reduced on the GPU (aggregate.c); 0 (default) = off */
    char *grid;             /* "grid": <xmin>,<ymax>,<dx>,<dy>,<nx>,<ny> (gcn10_parse_grid): no 10 m raster is written but
                               one raster per selected raster on that grid, the mean over each cell's pixels of all
                               blocks, reduced on the GPU (grid.c); absent (default) = off */
    char *storm;            /* "storm": <P>[,<lambda>] (gcn10_parse_storm): the design storm of the runoff-weighted
                               composites -- with grid, a second raster per selected raster, the runoff-equivalent CN of
                               every cell; with zonal, two more columns of the table; absent (default) = off */
    double storm_p, storm_lambda;   /* ... its rainfall depth in mm and its initial-abstraction ratio */
    char *storms;           /* "storms": <P1>[:<P2>...][,<lambda>] (gcn10_parse_storms): a ladder of 1 to GCN10_MAX_STORMS
                               design storms in one grid or zonal run -- per storm what "storm" gives for one; not
                               together with "storm"; absent (default) = off */
    int n_storms;           /* ... how many, */
    double storms_p[GCN10_MAX_STORMS];      /* their rainfall depths in mm, rising, */
    double storms_lambda;   /* and the initial-abstraction ratio of all of them */
    char *rain;             /* "rain": a one-band Byte GeoTIFF of nx x ny pixels, the rainfall depth of every cell of
                               "grid" in counts (gcn10_rain_load); not together with "storm" / "storms"; absent = off */
    char *rain_unit;        /* "rain_unit": <unit>[,<lambda>] (gcn10_parse_rain_unit): millimetres per count (default 1)
                               and the initial-abstraction ratio (default 0.2); needs "rain" */
    char *zone_rain;        /* "zone_rain": a one-band Byte GeoTIFF with a geotransform, the rainfall depth in counts under
                               the zones of a zonal run (gcn10_zone_rain_load); not together with "storm" / "storms";
                               absent = off */
    char *zone_rain_unit;   /* "zone_rain_unit": <unit>[,<lambda>] as "rain_unit"; needs "zone_rain" or "zone_rains" */
    char *rains;            /* "rains": <file1>[:<file2>...] (gcn10_parse_rains): 1 to GCN10_MAX_RAINS rainfall rasters as
                               "rain" takes one, all in one grid run that counts its pixels once; "rain_unit" holds for
                               all of them; not together with "rain"; absent = off */
    char *zone_rains;       /* "zone_rains": <file1>[:<file2>...] (gcn10_parse_rains): 1 to GCN10_MAX_RAINS rainfall rasters
                               as "zone_rain" takes one, all in one zonal run that counts its pixels once (gcn10_zone_rains_load);
                               "zone_rain_unit" holds for all of them; not together with "zone_rain"; absent = off */
    char *runoff_rain;      /* "runoff_rain": a one-band Byte GeoTIFF with a geotransform, the rainfall depth in counts; the
                               run writes the runoff depth of every pixel instead of its curve number ("Runoff rasters under
                               a rainfall raster" below); absent = off */
    char *runoff_rain_unit; /* "runoff_rain_unit": <unit>[,<lambda>] as "rain_unit"; needs "runoff_rain" */
    char *runoff_unit;      /* "runoff_unit": <mm> per count of the written rasters (gcn10_parse_runoff_unit; default: the
                               rain unit); needs "runoff_rain" */
} gcn10_config;

enum { GCN10_COMPRESS_DEFLATE = 0, GCN10_COMPRESS_LZW = 1 };
enum { GCN10_OVERVIEW_NEAREST = 0, GCN10_OVERVIEW_AVERAGE = 1 };

/* "g_ii", "p_i,f_iii", "all" -> table mask; "drained" | "undrained" | "both" | "all" -> condition mask.
 * Return 0 and set *mask, or -1 for a name that is not a lookup / condition. */
int gcn10_parse_lookups(const char *text, unsigned *mask);
int gcn10_parse_conditions(const char *text, unsigned *mask);
/* "deflate" | "lzw" (any case) -> GCN10_COMPRESS_*.  0, or -1 for another name. */
int gcn10_parse_compress(const char *text, int *codec);
/* "nearest" | "average" (any case) -> GCN10_OVERVIEW_*; "0" | "1" -> cog.  0, or -1 for another value. */
int gcn10_parse_overview_resampling(const char *text, int *method);
int gcn10_parse_cog(const char *text, int *cog);
/* "0" | "1" -> stats; "none" (any case) -> -1 | an integer 0..255 -> nodata.  0, or -1 for another value. */
int gcn10_parse_stats(const char *text, int *stats);
int gcn10_parse_nodata(const char *text, int *nodata);
int gcn10_parse_verify(const char *text, int *verify);      /* "0" | "1".  0, or -1 for another value. */
int gcn10_parse_zonal(const char *text, int *zonal);        /* "0" | "1".  0, or -1 for another value. */
/* "0" (off) | an integer 2..256 -> aggregate.  0, or -1 for another value. */
int gcn10_parse_aggregate(const char *text, int *factor);

/* Returns 0; -1 cannot open (message in err); -3 a bad "lookups" / "conditions" / "compress" / "cog" /
 * "overview_resampling" / "stats" / "nodata" / "verify" / "zonal" / "zones_id_field" / "aggregate" / "grid" / "storm" / "storms" / "rain_unit" / "zone_rain_unit" / "rains" / "runoff_rain_unit" / "runoff_unit" value; -2 a required key is missing
 * (the reference aborts in both cases, src/config.c:50-54, 107-113). */
int gcn10_config_parse(const char *path, gcn10_config *cfg, char *err, size_t errcap);
void gcn10_config_free(gcn10_config *cfg);

/* Per-worker log, "<log_dir>/rank_<r>.log", append mode, lines
 * "[%Y-%m-%dT%H:%M:%S] [LEVEL] [rank r] msg" (src/log.c:67-86, 149-166).
 * A "rank" is a GPU worker here.  Thread safe. */
typedef struct gcn10_log gcn10_log;
gcn10_log *gcn10_log_open(const char *log_dir, int rank);       /* = init_logging  */
void gcn10_log_message(gcn10_log *lg, const char *level, const char *msg,
                       bool also_console);                      /* = log_message   */
void gcn10_log_close(gcn10_log *lg);                            /* = finalize_logging */

/* ------------------------------------------------------------------------ */
/* block index (src/raster.c:23-103, src/cn.c:155-184)                      */
/* ------------------------------------------------------------------------ */

/* Whitespace-separated integers; parsing stops at the first token that is not
 * an integer (fscanf("%d"), src/raster.c:46).  Returns a malloc'd array. */
int *gcn10_read_block_list(const char *path, int *n_blocks);

/* The polygon shapefile of block extents, read without OGR: the .shp record
 * bounding boxes and the "ID" column of the .dbf. */
typedef struct gcn10_blocks {
    int n;
    int *id;                /* "ID" attribute of every feature, file order   */
    double (*bbox)[4];      /* {minx, miny, maxx, maxy} = OGR envelope       */
} gcn10_blocks;

int gcn10_blocks_open(const char *shp_path, gcn10_blocks *out, char *err, size_t errcap);
void gcn10_blocks_free(gcn10_blocks *b);
/* First feature whose ID equals block_id (the reference's attribute filter +
 * first feature, src/cn.c:162-171); returns its index or -1. */
int gcn10_blocks_find(const gcn10_blocks *b, int block_id);

/* ------------------------------------------------------------------------ */
/* rasters (src/raster.c:106-227) without GDAL                               */
/* ------------------------------------------------------------------------ */

typedef struct gcn10_raster gcn10_raster;   /* an open GeoTIFF or VRT, 1 band, Byte */

/* GeoTIFF (classic or BigTIFF; strips or tiles; none / LZW / DEFLATE /
 * PackBits; predictor 1 or 2) or a VRT mosaic of such files. */
gcn10_raster *gcn10_raster_open(const char *path, const char *vrt_tile_dir,
                                char *err, size_t errcap);
void gcn10_raster_close(gcn10_raster *r);
void gcn10_raster_info(const gcn10_raster *r, int *xsize, int *ysize, double gt[6]);
/* Rows [yoff, yoff+ycount) x columns [xoff, xoff+xcount) into dst (row-major,
 * xcount bytes per row).  Thread safe per raster handle.  0 or -1. */
int gcn10_raster_read(gcn10_raster *r, int xoff, int yoff, int xcount, int ycount,
                      uint8_t *dst, char *err, size_t errcap);

/* Georeferencing tags an output inherits from the landcover input (the
 * reference copies the input's WKT, src/raster.c:212-214). */
typedef struct gcn10_georef {
    uint16_t *geokeys;      /* GeoKeyDirectoryTag (34735) */
    int n_geokeys;
    double *geodoubles;     /* GeoDoubleParamsTag (34736) */
    int n_geodoubles;
    char *geoascii;         /* GeoAsciiParamsTag (34737), NUL terminated */
} gcn10_georef;
const gcn10_georef *gcn10_raster_georef(const gcn10_raster *r);

/* Streaming writer of one tiled DEFLATE GeoTIFF (GTiff, COMPRESS=DEFLATE,
 * TILED=YES -> 256x256 tiles, Byte, 1 band; src/raster.c:204-209).  Tiles may
 * be handed over already compressed (zlib streams), in any order. */
typedef struct gcn10_tiff_writer gcn10_tiff_writer;
gcn10_tiff_writer *gcn10_tiff_create(const char *path, int xsize, int ysize,
                                     const double gt[6], const gcn10_georef *georef,
                                     char *err, size_t errcap);
int gcn10_tiff_tiles_across(const gcn10_tiff_writer *w);
int gcn10_tiff_tiles_down(const gcn10_tiff_writer *w);
/* Appends one compressed tile (tx, ty) of `nbytes` zlib-stream bytes. */
int gcn10_tiff_put_tile(gcn10_tiff_writer *w, int tx, int ty, const void *zdata, size_t nbytes);
/* n tiles of the raster in one go (gathered writes); same result as n gcn10_tiff_put_tile calls */
int gcn10_tiff_put_tiles(gcn10_tiff_writer *w, int n, const int *tx, const int *ty,
                         const void *const *zdata, const uint32_t *nbytes);
/* n tiles whose streams lie in one extent of memory (stream i at data + rel_off[i]): one write for all of
 * them.  What the GPU encoders produce for a raster and a strip. */
int gcn10_tiff_put_extent(gcn10_tiff_writer *w, const void *data, size_t extent_bytes, int n, const int *tx,
                          const int *ty, const uint32_t *rel_off, const uint32_t *nbytes);
/* TIFF Compression tag of the file: 8 (default, Adobe deflate: zlib streams) or 5 (LZW streams).  0 or -1. */
int gcn10_tiff_set_compression(gcn10_tiff_writer *w, int compression);
/* O_DIRECT for the tile data (config key "direct_io"): extents must then be 4096-aligned in memory and
 * readable to the next multiple of 4096.  0 = on, -1 = the file system refuses (nothing changed).  A put_tile or
 * put_tiles writes at unaligned positions and lengths: it turns O_DIRECT off for the rest of the file first. */
int gcn10_tiff_set_direct(gcn10_tiff_writer *w, bool on);
/* Cloud Optimized GeoTIFF (config key "cog"): the same raster plus n_levels overviews, in GDAL's COG layout --
 * the 8-byte header, GDAL's ghost area at offset 8 ("GDAL_STRUCTURAL_METADATA_SIZE=nnnnnn bytes", LAYOUT=
 * IFDS_BEFORE_DATA, BLOCK_ORDER=ROW_MAJOR, KNOWN_INCOMPATIBLE_EDITION=NO; no block leader or trailer), then
 * every IFD with its values (full resolution first, then levels 1 .. n_levels, chained in that order), then the
 * tile data.  Level k is ceil(xsize / 2^k) x ceil(ysize / 2^k) pixels in 256x256 tiles; its IFD has
 * NewSubfileType = 1 and no geo tags.  The IFDs' room is reserved here (tile counts are known) and filled in by
 * gcn10_tiff_finish.  Tile data must arrive in file order: level n_levels first, full resolution last, and within
 * a level in row-major tile order; a put that would break that order returns -1 and writes nothing (the file
 * stays usable).  Extents, gathered puts, direct I/O, .part + rename and Compression 5 work as for a plain file. */
#define GCN10_COG_MAX_LEVELS 8      /* the program's limit: windows of at most 65536 px (gcn10_gpu_overview_average) */
gcn10_tiff_writer *gcn10_tiff_create_cog(const char *path, int xsize, int ysize, const double gt[6],
                                         const gcn10_georef *georef, int n_levels, char *err, size_t errcap);
/* The COG rule with BLOCKSIZE = 256: the smallest k >= 0 with ceil(xsize / 2^k) <= 256 and ceil(ysize / 2^k) <= 256
 * (-1 for a bad size). */
int gcn10_cog_levels(int xsize, int ysize);
/* Level `level` of a COG writer (0 = the full-resolution raster, the writer itself) as a writer for the put calls
 * and gcn10_tiff_tiles_across / _down; owned by the file's writer (finish / abort it, not the view).  NULL for a
 * level the file does not have. */
gcn10_tiff_writer *gcn10_tiff_level(gcn10_tiff_writer *w, int level);
int gcn10_tiff_n_levels(const gcn10_tiff_writer *w);   /* 0 for a plain file */
/* GDAL's NoData and metadata tags (config keys "nodata" and "stats"), beside the geo tags in ascending tag order.
 * gcn10_tiff_set_nodata: GDAL_NODATA (42113, ASCII, e.g. "255") on every IFD, COG overviews included, as GDAL
 *   writes it; v in 0..255.
 * gcn10_tiff_set_metadata_xml: GDAL_METADATA (42112, ASCII, NUL terminated) of the full-resolution IFD only, as
 *   GDAL's COG driver writes it; a copy is kept, NULL removes it.
 * gcn10_tiff_reserve_metadata: a COG's directories are laid out at create, so the room of the metadata value must be
 *   known before its text is: `bytes` (including the NUL) are kept free for it, and the tag is then always written
 *   (an empty <GDALMetadata> element when no text is set by finish).  Nothing to do for a plain file.
 * On a plain file all three may be called at any time before gcn10_tiff_finish.  On a COG, set_nodata and
 * reserve_metadata change the directories' size and must come before the first tile (-1 otherwise), and a text
 * longer than the reserved room is refused (-1).  0 or -1. */
int gcn10_tiff_set_nodata(gcn10_tiff_writer *w, int v);
int gcn10_tiff_set_metadata_xml(gcn10_tiff_writer *w, const char *xml);
int gcn10_tiff_reserve_metadata(gcn10_tiff_writer *w, size_t bytes);
/* Writes the directory and closes the file.  0 or -1. */
int gcn10_tiff_finish(gcn10_tiff_writer *w, char *err, size_t errcap);
void gcn10_tiff_abort(gcn10_tiff_writer *w);

/* zlib-compresses one 256x256 tile cut from a raster strip (rows are `stride`
 * bytes apart; the part of the tile outside the raster is zero-filled as GDAL
 * pads edge tiles).  Returns the compressed size or 0 on error. */
size_t gcn10_deflate_tile(const uint8_t *src, size_t stride, int valid_w, int valid_h,
                          int level, uint8_t *dst, size_t dstcap);

/* Convenience: whole raster in memory -> file (the reference's save_raster
 * signature, src/raster.c:192-194).  0 or -1. */
int gcn10_save_raster(const uint8_t *data, int xsize, int ysize, const double gt[6],
                      const gcn10_georef *georef, const char *path, int level,
                      char *err, size_t errcap);


/* ------------------------------------------------------------------------ */
/* band statistics (config keys "stats", "nodata"): no counterpart in the reference                         */
/* ------------------------------------------------------------------------ */

/* The histogram of one raster from a block's (landcover, soil code) pair histogram (gcn10_gpu_pair_histogram:
 * pair[bin * 256 + landcover], codes[bin] = the soil code of each of the 16 bins, gcn10_gpu_pair_histogram_codes).
 * The value of a pair is the kernels' own: plane = the code's drained (low nibble) or undrained (high nibble)
 * plane, table[landcover][plane] if plane < 5 and that value is < 255 (stored through a (uint8_t) cast), else 255
 * (src/cn.c:114-131).  hist[v] for v in 0..255 is overwritten. */
void gcn10_raster_histogram(const uint64_t *pair, const uint8_t codes[16], const int table[256][5], int drained,
                            uint64_t hist[256]);

/* Statistics of a histogram as GDAL's ComputeStatistics makes them for a Byte band: the valid pixels are all of
 * them, or all but the value `nodata` (0..255; -1 = none); min and max over them, the plain mean, the population
 * standard deviation sqrt(n * sum(v^2) - sum(v)^2) / n from exact integer sums, valid percent = 100 * valid / total. */
typedef struct gcn10_band_stats {
    uint64_t total, valid;
    int min, max;
    double mean, stddev, valid_percent;
} gcn10_band_stats;
void gcn10_band_stats_of(const uint64_t hist[256], int nodata, gcn10_band_stats *st);

/* GDAL_METADATA text of the statistics, the way GDAL writes band statistics into a GeoTIFF:
 *   <GDALMetadata>\n  <Item name="STATISTICS_MAXIMUM" sample="0">98</Item>\n ... </GDALMetadata>\n
 * items in GDAL's (sorted) order MAXIMUM, MEAN, MINIMUM, STDDEV, VALID_PERCENT; min, max, mean and stddev as
 * "%.14g", the valid percent as "%.4g" (GDALRasterBand::SetStatistics / ComputeStatistics).  Returns the length
 * without the NUL, or 0 when the raster has no valid pixel (GDAL computes no statistics then: no items, no text)
 * or the text does not fit cap.  GCN10_STATS_XML_MAX bytes always suffice. */
#define GCN10_STATS_XML_MAX 512
size_t gcn10_stats_xml(const gcn10_band_stats *st, char *buf, size_t cap);

/* ------------------------------------------------------------------------ */
/* zones (config keys "zonal", "zones_shp_path"): no counterpart in the reference                           */
/* ------------------------------------------------------------------------ */

/* A polygon shapefile of zones (watersheds, counties, ...), read without OGR: shape types 5, 15 and 25 (Z and M are
 * ignored) with any number of parts; a null shape (type 0) is a zone without pixels; any other type is an error that
 * names the record.  id[i] is the numeric .dbf field `id_field` (NULL = "ID", matched without case) of record i;
 * duplicates are allowed.  The files are untrusted: every length, count and offset is checked against the file size,
 * part offsets must start at 0 and ascend inside the point array, and coordinates must be finite.
 * Ring k (over all records) is the points ring_pt[k] .. ring_pt[k + 1]; record i has the rings ring_first[i] ..
 * ring_first[i + 1].  A ring whose last point is not its first is closed by the reader's users. */
typedef struct gcn10_zones {
    int n;                  /* records = zones, file order */
    int64_t *id;
    double (*bbox)[4];      /* {minx, miny, maxx, maxy} of the record's points (the header's box is not believed); all zero for a null shape */
    uint64_t *ring_first;   /* [n + 1] */
    uint64_t *ring_pt;      /* [n_rings + 1] */
    double *xy;             /* [n_points][2] */
    uint64_t n_rings, n_points;
} gcn10_zones;
int gcn10_zones_open(const char *shp_path, const char *id_field, gcn10_zones *out, char *err, size_t errcap);
void gcn10_zones_free(gcn10_zones *z);

/* Spans of zone pixels and the work items of gcn10_gpu_zonal_pair_histogram (the same structs as in gcn10_gpu.h). */
#ifndef GCN10_ZONE_SPAN_DEFINED
#define GCN10_ZONE_SPAN_DEFINED
typedef struct gcn10_zone_span { int32_t y, x0, x1, zone; } gcn10_zone_span;       /* columns [x0, x1) of row y */
typedef struct gcn10_zone_item { uint32_t first_span, n_spans; } gcn10_zone_item;
#endif

/* Scan conversion of the zones over one block.  The block has the clipped geotransform gt (gcn10_raster_window;
 * north up: gt[1] > 0, gt[5] < 0, no rotation) and W x H pixels; pixel (x, y) has the centre
 *   px = gt[0] + (x + 0.5) * gt[1],  py = gt[3] + (y + 0.5) * gt[5]     (IEEE double, this order, no FMA).
 * Membership: an edge (x1,y1)-(x2,y2) of any ring of the zone crosses row y iff (y1 <= py) != (y2 <= py).  The
 * crossing is evaluated from the edge's lower endpoint, whichever way the ring runs: with (xl,yl) the endpoint of
 * smaller y and (xh,yh) the other (a horizontal edge crosses no row, so one y is smaller),
 *   xc = xl + (py - yl) * (xh - xl) / (yh - yl)                         (IEEE double, this order, no FMA);
 * with the row's crossings sorted c0 <= c1 <= ..., the pixel is in the zone iff c[2i] <= px < c[2i+1] for some i
 * (even-odd: holes and nested parts need no special case).  Two zones that share an edge, one ring running it P->Q
 * and the other Q->P, compute the same double for it, so a pixel whose centre lies on the edge is in exactly one of
 * them: zones that tile an area count each of its pixels once.
 * Ownership: only pixels with own[0] <= px < own[2] and own[1] < py <= own[3] are counted (own = the block's
 * shapefile bounding box {minx, miny, maxx, maxy}; NULL = every pixel of the window), so that blocks whose windows
 * overlap count every pixel once.
 * Result: the local zones (records whose bounding box meets the block and that own at least one pixel there), their
 * spans sorted by (zone = local index, y, x0), never empty and never longer than max_span_px, and items of
 * consecutive spans of one zone covering at most max_item_px pixels each (0 = the built-in bounds; results never
 * depend on them).  Cost: O(edges + rows touched + crossings) per zone.  0, or -1 with a message. */
typedef struct gcn10_zone_plan {
    int n_local;
    int32_t *local_zone;        /* [n_local] record index of each local zone, ascending */
    uint64_t *local_pixels;     /* [n_local] pixels of its spans */
    size_t n_spans, n_items;
    gcn10_zone_span *spans;
    gcn10_zone_item *items;
} gcn10_zone_plan;
int gcn10_zones_build_plan(const gcn10_zones *z, const double gt[6], int W, int H, const double own[4],
                           uint32_t max_span_px, uint32_t max_item_px, gcn10_zone_plan *out, char *err,
                           size_t errcap);
void gcn10_zone_plan_free(gcn10_zone_plan *p);
/* The item rule alone, over spans already sorted by (zone, y, x0): splits spans longer than max_span_px, then groups
 * them.  out->spans and out->items are filled (the local_* arrays stay empty).  0 or -1 (out of memory, or a span
 * with x0 >= x1). */
int gcn10_zone_items_build(const gcn10_zone_span *spans, size_t n_spans, uint32_t max_span_px, uint32_t max_item_px,
                           gcn10_zone_plan *out);

/* ------------------------------------------------------------------------ */
/* aggregated rasters (config key "aggregate", --aggregate): no counterpart in the reference                */
/* ------------------------------------------------------------------------ */

/* The grid of f x f landcover pixels a block's aggregated rasters live on.  The block has W x H pixels and the clipped
 * geotransform gt (gcn10_raster_window; north up, no rotation); own = its shapefile bounding box {minx, miny, maxx,
 * maxy}, NULL = every pixel.  [x0, x1) x [y0, y1) is the owned pixel rectangle by the ownership rule of
 * gcn10_zones_build_plan (pixel centres gt[0] + (x + 0.5) * gt[1], gt[3] + (y + 0.5) * gt[5] with own[0] <= px <
 * own[2], own[1] < py <= own[3]); cell (cx, cy) covers columns x0 + cx f .. min(x0 + (cx + 1) f, x1) - 1 and rows
 * likewise, so Wa = ceil((x1 - x0) / f), Ha = ceil((y1 - y0) / f), and no cell is shared between blocks.  The
 * geotransform of the Wa x Ha raster, in IEEE double, this order, no FMA:
 *   out_gt[0] = gt[0] + x0 * gt[1];  out_gt[3] = gt[3] + y0 * gt[5];  out_gt[1] = f * gt[1];  out_gt[5] = f * gt[5];
 *   out_gt[2] = out_gt[4] = 0.
 * 0; -1 for f outside 2..256, a block that is not north up, or one that owns no pixel. */
typedef struct gcn10_aggregate_geom {
    int x0, x1, y0, y1;
    int Wa, Ha;
    double gt[6];
} gcn10_aggregate_geom;
int gcn10_aggregate_geometry(int W, int H, const double gt[6], const double own[4], int f, gcn10_aggregate_geom *out);

/* ------------------------------------------------------------------------ */
/* model grid (config key "grid", --grid): no counterpart in the reference                                  */
/* ------------------------------------------------------------------------ */

/* A grid of nx x ny cells of dx x dy CRS units in the landcover's CRS; (xmin, ymax) is the outer upper-left corner of
 * cell (0, 0).  Cell edges, in IEEE double, this order, no FMA:
 *   ex(k) = xmin + (double)k * dx,   ey(k) = ymax - (double)k * dy.
 * A pixel with centre (px, py) -- the centres of gcn10_zones_build_plan -- is in cell column k iff ex(k) <= px < ex(k+1)
 * and in cell row k iff ey(k+1) < py <= ey(k): the half-open sides of the ownership rule, so a centre on an edge is in
 * exactly one cell; outside [0, nx) x [0, ny) it is in none. */
typedef struct gcn10_grid {
    double xmin, ymax, dx, dy;
    int nx, ny;
} gcn10_grid;
#define GCN10_GRID_MAX_CELLS (1 << 26)
/* "<xmin>,<ymax>,<dx>,<dy>,<nx>,<ny>": four doubles (strtod) and two integers, nothing else; all finite, dx, dy > 0,
 * nx, ny >= 1, nx * ny <= GCN10_GRID_MAX_CELLS.  0, or -1 for another text. */
int gcn10_parse_grid(const char *text, gcn10_grid *out);

/* One block on the grid.  The block has W x H pixels and the clipped geotransform gt (north up, no rotation); own = its
 * shapefile bounding box {minx, miny, maxx, maxy} (NULL: every pixel of the window is owned, and no cell is known to
 * be complete).  [x0, x1) x [y0, y1) is the owned pixel rectangle (gcn10_owned_window's); [cx0, cx1) x [cy0, cy1) the
 * cells that hold an owned pixel, empty (cx0 == cx1 == cy0 == cy1 == 0, no arrays) when there is none.  cellx[W] and
 * celly[H]: the LOCAL cell column k - cx0 and row k - cy0 of every pixel column and row, -1 for one that is not owned
 * or lies outside the grid; the non-negative entries never decrease.  The index k is found by a division and then
 * corrected with the rule's own comparisons: the comparisons decide.  complete_x[cx1 - cx0]: own[0] <= ex(k) and
 * ex(k+1) <= own[2]; complete_y[cy1 - cy0]: own[1] <= ey(k+1) and ey(k) <= own[3] -- every centre the cell column or
 * row can hold is owned by this block.  A cell is complete iff its column and its row are; the others are shared
 * (another block may add to them), and shared[n_shared] lists their local indices (cy - cy0) * (cx1 - cx0) + cx - cx0,
 * ascending.  0; -1 for a bad size, a block that is not north up, or out of memory. */
typedef struct gcn10_grid_plan {
    int x0, x1, y0, y1;
    int cx0, cx1, cy0, cy1;
    int32_t *cellx, *celly;
    uint8_t *complete_x, *complete_y;
    uint32_t *shared;
    size_t n_shared;
} gcn10_grid_plan;
int gcn10_grid_plan_block(const gcn10_grid *g, int W, int H, const double gt[6], const double own[4],
                          gcn10_grid_plan *out);
void gcn10_grid_plan_free(gcn10_grid_plan *p);

/* ------------------------------------------------------------------------ */
/* runoff-weighted composites (config key "storm", --storm): no counterpart in the reference                */
/* ------------------------------------------------------------------------ */

/* "<P>[,<lambda>]": the rainfall depth of a design storm in mm and its initial-abstraction ratio (absent: 0.2), read
 * with strtod, nothing else in the text; 0 < P <= 650 and 0 <= lambda < 1.  0, or -1 for another text. */
int gcn10_parse_storm(const char *text, double *P, double *lambda);
/* "<P1>[:<P2>...][,<lambda>]": 1 to GCN10_MAX_STORMS rainfall depths and one ratio for all of them, every field read
 * as gcn10_parse_storm reads its own.  The depths rise in hundredths of a millimetre: N_k = q_k[100] of
 * gcn10_runoff_table(P_k, lambda) is strictly increasing (the file names and the columns carry N, so no two storms
 * share a name).  0 with *k depths in P, or -1 for another text (nothing is written then). */
int gcn10_parse_storms(const char *text, double P[GCN10_MAX_STORMS], int *k, double *lambda);
/* The runoff depth of every raster value for that storm, in units of 0.01 mm.  q[0] = q[255] = 0; for v in 1..254, in
 * IEEE double, this order, no FMA:
 *   c = min(v, 100);  S = 25400.0 / c - 254.0;  Ia = lambda * S;
 *   !(P > Ia): q[v] = 0;  else  e = P - Ia,  q[v] = floor(e * e / (e + S) * 100.0 + 0.5).
 * Table values above 100 count as 100; q[100] = round(100 P) <= 65000 is the maximum of the table. */
void gcn10_runoff_table(double P, double lambda, uint16_t q[256]);
/* The runoff-equivalent curve number of a cell (or zone): over its pixels with value v != 255, s = the sum of v, n
 * their count, sw = the sum of q[v].  n == 0: 255.  sw == 0: the mean byte (2 s + n) / (2 n) -- no pixel sheds water,
 * every CN up to the storm's threshold is "equivalent", and the mean is one of them.  Otherwise the smallest c in
 * 1..100 with n * q[c] >= sw, in 64-bit integers (100 when there is none, which cannot happen with a table of
 * gcn10_runoff_table: q[100] is its maximum). */
int gcn10_runoff_cn(uint64_t s, uint64_t n, uint64_t sw, const uint16_t q[256]);

/* A rainfall raster on the model grid (config key "rain", --rain): a rainfall depth per cell instead of one per run.
 * The raster holds one byte b per cell of the grid, and the cell's storm is P = b * unit mm: all 256 bytes are depths,
 * there is no NoData value, and b = 0 is "no rain" (its table is all zero, so sw = 0 and the cell gets its mean byte by
 * the rule of gcn10_runoff_cn).  cnq_<hc>_<arc>_rain.tif holds gcn10_runoff_cn(s, n, sw, q[b]) per cell, {s, n, sw} as
 * for one storm with sw = the sum of q[b][v] over the cell's pixels. */
/* "<unit>[,<lambda>]": millimetres per count and the initial-abstraction ratio (absent: 0.2), every field read as
 * gcn10_parse_storm reads its own; 0 < unit, 255 * unit <= 650 and 0 <= lambda < 1.  0, or -1 for another text. */
int gcn10_parse_rain_unit(const char *text, double *unit, double *lambda);
/* q[b] = gcn10_runoff_table(b * unit, lambda) for b = 0..255, and nothing else: 128 KiB, made once per run. */
void gcn10_rain_tables(double unit, double lambda, uint16_t q[256][256]);
/* Reads the rainfall raster of grid g whole: *out = nx * ny bytes, row major (the caller frees them).  The file has
 * exactly nx x ny pixels; if it carries a geotransform, its origin and pixel size equal xmin, ymax, dx, -dy of the grid
 * as doubles, bit for bit, and it has no rotation; a file without georeferencing (the reader then reports the
 * geotransform 0, 1, 0, 0, 0, 1) is taken to lie on the grid.  Returns 0, or GCN10_RAIN_E_* with the message of the
 * run's refusal in err ("rain: cannot read '<file>': ...", "rain: '<file>' has <w> x <h> pixels, the grid has <nx> x
 * <ny> cells", "rain: '<file>' does not lie on the grid (origin %.17g, %.17g, pixel %.17g x %.17g)"). */
enum { GCN10_RAIN_E_READ = -1, GCN10_RAIN_E_SIZE = -2, GCN10_RAIN_E_GEOTRANSFORM = -3 };
int gcn10_rain_load(const char *path, const gcn10_grid *g, uint8_t **out, char *err, size_t errcap);

/* Per-pixel runoff depth under a rainfall raster (config key "runoff_rain", --runoff-rain): the tables of
 * gcn10_rain_tables as bytes of an output unit.  u: the unit in hundredths of a millimetre per count, u >= 1.  Integers
 * only: t[b][255] = 255 (no value stays no value); for v < 255, t[b][v] = min(254, (2 * q[b][v] + u) / (2 * u)): round
 * half up, saturating at 254.  q[b][v] <= q[b][100] = round(100 * b * unit), so with u = the rain unit in hundredths no
 * entry of a table b < 255 saturates: its largest is b.  (Table 255 alone does: its largest entry would be 255.) */
void gcn10_runoff_bytes(const uint16_t q[256][256], unsigned u, uint8_t t[256][256]);
/* "<mm>": the output unit in millimetres per count, one field read as gcn10_parse_storm reads its own;
 * *u = floor(100 * x + 0.5) in plain IEEE double, accepted iff 1 <= *u <= 65000.  0, or -1 for another text. */
int gcn10_parse_runoff_unit(const char *text, unsigned *u);
/* The output unit that stands for a rain unit of `mm` millimetres per count: floor(100 * mm + 0.5) by the same
 * arithmetic, at least 1 (the default of "runoff_unit"). */
unsigned gcn10_runoff_unit_of(double mm);

/* Runoff rasters under a rainfall raster (config keys "runoff_rain", "runoff_rain_unit", "runoff_unit"; --runoff-rain,
 * --runoff-rain-unit, --runoff-unit): a sixth kind of run, which writes for every block and selected raster
 *     runoff_rasters_<cond>/q_<hc>_<arc>_<id>.tif
 * with the size, geotransform, tiling, tags and overwrite rule of the block's CN raster.  The rainfall raster follows the
 * rules of "zone_rain" (one Byte band, north-up geotransform, the landcover's CRS, at most GCN10_GRID_MAX_CELLS pixels;
 * it IS a gcn10_grid; messages under "runoff_rain:") and is read once, before any GPU is opened.  A pixel's rain cell is
 * the one gcn10_grid_plan_block(grid, W, H, gt_block, NULL, ...) names: there is no ownership box, every pixel of the
 * window is written.  The value of a pixel with curve number v (what the CN raster holds) under a cell of byte b is
 *     t[b][v],  t = gcn10_runoff_bytes(gcn10_rain_tables(unit, lambda), u),
 * that is the runoff depth Q(b * unit, v) in counts of u / 100 mm, rounded half up, at most 254; 255 where the CN raster
 * holds 255 and where the pixel lies in no rain cell.  A block that meets no rain cell still writes its files, all 255.
 * Allowed with it: compress=lzw, nodata, lookups, conditions, direct_io, -l, -o, launcher ranks.  Refused, each with
 * one "[rank 0] runoff_rain cannot be combined with <what>" line before any GPU is opened, tested in THIS order:
 *     --verify, aggregate, --zonal, grid, storm, storms, rain, rains, zone_rain, zone_rains, cog, stats
 * (the last two compute from CN, not from these bytes); before them "runoff_rain_unit needs runoff_rain" and
 * "runoff_unit needs runoff_rain", then the bad values of the two units, then the raster's own four messages. */

/* Several rainfall rasters in one grid run (config key "rains", --rains): K = 1 to GCN10_MAX_RAINS files, each by every
 * rule of "rain", one unit and one set of 256 tables (gcn10_rain_tables) for all -- only the byte of a cell differs from
 * layer to layer.  The pixels of a block are counted once: the sums carry 2 + K words per (raster, cell), word 2 + j the
 * sum of q[b_j][v] with b_j the cell's byte in file j.  With one file the run writes what "rain" writes, byte for byte
 * and name for name; with K > 1, cnq_<hc>_<arc>_rain<j>.tif for j = 1..K in the order given, each the file "rain" alone
 * writes for file j, and the means are those of the run without rain. */
#define GCN10_MAX_RAINS 8
/* "<file1>[:<file2>...]": 1 to GCN10_MAX_RAINS file names separated by ':' (so a name holds none), none of them empty.
 * 0 with *copy = the text with every ':' replaced by a NUL (the caller frees it), files[0 .. *k) pointing into it; or -1
 * for NULL, an empty text, an empty member or more than GCN10_MAX_RAINS members (nothing is written or allocated then),
 * and for no memory. */
int gcn10_parse_rains(const char *text, char **copy, const char *files[GCN10_MAX_RAINS], int *k);
/* gcn10_rain_load for every file, in order: out[0 .. k) = nx * ny bytes each (the caller frees them).  Returns 0, or the
 * GCN10_RAIN_E_* of the first file that fails, with gcn10_rain_load's message under the prefix "rains:" in err; nothing
 * stays allocated then and out[] is all NULL. */
int gcn10_rains_load(const char *const files[], int k, const gcn10_grid *g, uint8_t *out[GCN10_MAX_RAINS], char *err,
                     size_t errcap);
/* The bytes of one cell from its 2 + k words {s, n, sw_1 .. sw_k} (a cell that several blocks added to, after the last
 * block): cn[j] = gcn10_runoff_cn(s, n, sw_j, q[bytes[j]]), bytes[j] the cell's byte in layer j. */
void gcn10_rains_cell(const uint64_t *words, int k, const uint8_t bytes[], const uint16_t q[256][256], uint8_t cn[]);

/* A rainfall raster under the zones (config keys "zone_rain" and "zone_rain_unit", --zone-rain / --zone-rain-unit; needs
 * zones): the runoff of every zone under a depth that varies across it.  "rain" stays "one byte per cell of grid" and
 * stays refused with zones; this raster carries its own georeferencing.
 *
 * The raster: one Byte band WITH a geotransform, north up and without rotation (gt[1] > 0, gt[5] < 0, gt[2] == gt[4] ==
 * 0), taken to be in the landcover's CRS, of at most GCN10_GRID_MAX_CELLS pixels.  It IS the gcn10_grid {xmin = gt[0],
 * ymax = gt[3], dx = gt[1], dy = -gt[5], nx, ny}: a landcover pixel's rain cell is decided by that grid's rule, through
 * gcn10_grid_plan_block(grid, W, H, gt_block, NULL, ...) (ownership is already in the zone's spans).  Byte b means P =
 * b * unit mm with table q[b] of gcn10_rain_tables(unit, lambda); b = 0 is no rain; there is no NoData byte.  The unit
 * is read by gcn10_parse_rain_unit (defaults 1 mm and 0.2).
 *
 * The sums, for zone z and selected raster r, over the pixels of z (the spans of gcn10_zones_build_plan, unchanged)
 * that lie in a rain cell and whose value v != 255:  s = the sum of v, n = their count, sw = the sum of q[b(pixel)][v];
 * independent of r: rain_pixels = the pixels of z that lie in a rain cell, rain_sum = the sum of b over them.  All are
 * integers, additive across blocks and workers.
 *
 * zonal_cn.csv keeps its columns, byte for byte, and gains rain_pixels,rain_mm,rain_valid,runoff_mm_rain,cn_runoff_rain:
 *   rain_mm        = ((double)rain_sum / (double)rain_pixels) * unit, in this order; empty when rain_pixels == 0
 *   rain_valid     = n
 *   runoff_mm_rain = (double)sw / (double)n / 100.0, printed %.14g
 *   cn_runoff_rain = gcn10_runoff_cn(s, n, sw, T) with T = gcn10_runoff_table(rain_mm, lambda): the CN a lumped model
 *                    needs with the basin-mean depth to reproduce the distributed runoff
 * the last two empty when n == 0; with rain_mm == 0 the table is all zero and the rule gives the mean byte. */
/* The derived columns of one row: bit 0 of the result: *rain_mm holds (rain_pixels > 0); bit 1: *runoff_mm and *cn hold
 * (n > 0, which implies rain_pixels > 0).  What does not hold is 0, 0 and 255. */
int gcn10_zone_rain_values(uint64_t rain_pixels, uint64_t rain_sum, double unit, double lambda, uint64_t s, uint64_t n,
                           uint64_t sw, double *rain_mm, double *runoff_mm, int *cn);
/* Reads such a raster whole: *grid as above, *out = nx * ny bytes, row major (the caller frees them).  0, or -1 with the
 * run's refusal in err: "zone_rain: cannot read '<file>': ...", "zone_rain: '<file>' carries no geotransform" (the
 * reader reports 0, 1, 0, 0, 0, 1 then), "zone_rain: '<file>' is rotated or not north up", "zone_rain: '<file>' has
 * more than <GCN10_GRID_MAX_CELLS> pixels". */
int gcn10_zone_rain_load(const char *path, gcn10_grid *grid, uint8_t **out, char *err, size_t errcap);
/* The same reader with the four messages under another key's name ("<prefix>: cannot read ...", ...):
 * gcn10_zone_rain_load is this with prefix "zone_rain", a runoff_rain run passes "runoff_rain". */
int gcn10_rain_raster_load(const char *prefix, const char *path, gcn10_grid *grid, uint8_t **out, char *err,
                           size_t errcap);
/* The spans of a block's plan cut where the rainfall byte changes -- the input of gcn10_gpu_zonal_sums_rain (the same
 * item struct as in gcn10_gpu.h).  cellx[W], celly[H], cx0, cy0: the maps of gcn10_grid_plan_block for the block on the
 * raster's grid (column x lies in raster column cellx[x] + cx0; a negative entry: in none; both NULL: the block meets no
 * cell); rain: the raster's nx x ny bytes.  Each cut span is a maximal run of columns of ONE source span that have
 * cellx >= 0, in a row with celly >= 0, under one byte (neighbouring cells of equal byte merge), split at max_span_px;
 * spans sorted by (zone, byte, y, x0), their `zone` the plan's local index; items: runs of consecutive spans of ONE
 * zone and ONE byte (`table`), at most max_item_px pixels each (0 = the builder's own bounds; results never depend on
 * them).  rain_pixels[n_local], rain_sum[n_local]: the pixels of each local zone in a rain cell, and the sum of their
 * bytes.  Cost: O(W + spans + rain cells crossed), a counting sort on the byte within a zone.  0; -1 for a span outside
 * the W x H block, a zone outside the plan, or out of memory. */
#ifndef GCN10_ZONE_RAIN_ITEM_DEFINED
#define GCN10_ZONE_RAIN_ITEM_DEFINED
typedef struct gcn10_zone_rain_item { uint32_t first_span, n_spans, table, reserved; } gcn10_zone_rain_item;
#endif
typedef struct gcn10_zone_rain_plan {
    int n_local;
    uint64_t *rain_pixels, *rain_sum;   /* [n_local] */
    size_t n_spans, n_items;
    gcn10_zone_span *spans;
    gcn10_zone_rain_item *items;
} gcn10_zone_rain_plan;
int gcn10_zone_rain_cut(const gcn10_zone_plan *plan, int W, int H, const int32_t *cellx, const int32_t *celly, int cx0,
                        int cy0, const uint8_t *rain, int nx, int ny, uint32_t max_span_px, uint32_t max_item_px,
                        gcn10_zone_rain_plan *out);
void gcn10_zone_rain_plan_free(gcn10_zone_rain_plan *p);

/* Several rainfall rasters under the zones in one run (config key "zone_rains=<file1>[:<file2>...]", --zone-rains; read by
 * gcn10_parse_rains): K = 1 to GCN10_MAX_RAINS files, every one by every rule of "zone_rain" (Byte band, geotransform,
 * north up, at most GCN10_GRID_MAX_CELLS pixels); files 2..K have the size of file 1 and its geotransform, bit for bit.
 * One unit and lambda serve all layers ("zone_rain_unit" / --zone-rain-unit, accepted with either key), and so does one
 * set of gcn10_rain_tables.  Not together with "zone_rain", "storm" or "storms"; needs zones.
 *
 * The sums, for zone z and selected raster r, over the pixels of z that lie in a rain cell and whose value v != 255:
 * s = the sum of v and n = their count, both counted once; sw_j = the sum of q[b_j(pixel)][v] for each layer j.
 * Independent of r: rain_pixels, counted once (the grid is shared, so it is the same for every layer), and rain_sum_j per
 * layer.  All are integers, additive across blocks and workers.
 *
 * zonal_cn.csv: with K = 1, header and rows are byte for byte those of "zone_rain=<file1>".  With K > 1, after the columns
 * of the run without the key come rain_pixels,rain_valid and then, for j = 1..K in the order given,
 * rain_mm_rain<j>,runoff_mm_rain<j>,cn_runoff_rain<j>, each triple formed by gcn10_zone_rain_values(rain_pixels,
 * rain_sum_j, unit, lambda, s, n, sw_j, ...): as text what "zone_rain=<file_j>" alone prints in
 * rain_mm,runoff_mm_rain,cn_runoff_rain, empty fields included. */
/* gcn10_zone_rain_load for every file, in order: *grid of file 1, out[0 .. k) = nx * ny bytes each (the caller frees
 * them).  0, or -1 with the run's refusal in err: gcn10_zone_rain_load's message under the prefix "zone_rains:",
 * "zone_rains: '<file>' has <w> x <h> pixels, '<file1>' has <nx> x <ny>", or "zone_rains: '<file>' does not lie on the grid
 * of '<file1>' (origin %.17g, %.17g, pixel %.17g x %.17g)" with the file's own gt[0], gt[3], gt[1], gt[5]; nothing stays
 * allocated then, out[] is all NULL and *grid all zero. */
int gcn10_zone_rains_load(const char *const files[], int k, gcn10_grid *grid, uint8_t *out[GCN10_MAX_RAINS], char *err,
                          size_t errcap);
/* The spans of a block's plan cut wherever the byte of ANY of k layers changes -- the input of
 * gcn10_gpu_zonal_sums_rains (the same item struct as in gcn10_gpu.h).  It is the walk of gcn10_zone_rain_cut with "one
 * byte" replaced by "one k-tuple of bytes": rain[j] holds layer j's nx x ny bytes, k = 1..GCN10_MAX_RAINS; a tuple is 8
 * bytes, layer 0 first, bytes k..7 zero.  Each cut span is a maximal run of columns of ONE source span, in cells, under
 * one tuple (neighbouring cells of equal tuple merge), split at max_span_px; spans sorted by (zone, tuple, y, x0), tuples
 * in lexicographic order; items: runs of consecutive spans of ONE zone and ONE tuple (`table`), at most max_item_px pixels
 * each (0 = the builder's own bounds; results never depend on them).  rain_pixels[n_local]: the pixels of each local zone
 * in a rain cell; rain_sum[j][n_local]: the sum of layer j's bytes over them (rain_sum[j] is NULL for j >= k).  With k
 * identical layers, spans and items are those of gcn10_zone_rain_cut, with the byte repeated.  Cost: O(W + spans + rain
 * cells crossed + k * pieces), the counting sort of gcn10_zone_rain_cut once per layer, last layer first.  0; -1 for k
 * outside 1..GCN10_MAX_RAINS, a span outside the W x H block, a zone outside the plan, or out of memory. */
#ifndef GCN10_ZONE_RAINS_ITEM_DEFINED
#define GCN10_ZONE_RAINS_ITEM_DEFINED
typedef struct gcn10_zone_rains_item { uint32_t first_span, n_spans; uint8_t table[8]; } gcn10_zone_rains_item;
#endif
typedef struct gcn10_zone_rains_plan {
    int n_local, k;
    uint64_t *rain_pixels;                  /* [n_local] */
    uint64_t *rain_sum[GCN10_MAX_RAINS];    /* [k][n_local] */
    size_t n_spans, n_items;
    gcn10_zone_span *spans;
    gcn10_zone_rains_item *items;
} gcn10_zone_rains_plan;
int gcn10_zone_rains_cut(const gcn10_zone_plan *plan, int W, int H, const int32_t *cellx, const int32_t *celly, int cx0,
                         int cy0, const uint8_t *const rain[], int k, int nx, int ny, uint32_t max_span_px,
                         uint32_t max_item_px, gcn10_zone_rains_plan *out);
void gcn10_zone_rains_plan_free(gcn10_zone_rains_plan *p);

/* ------------------------------------------------------------------------ */
/* the run: src/main.c:58-203 + process_block, src/cn.c:134-384              */
/* ------------------------------------------------------------------------ */

typedef struct gcn10_run_options {
    const char *config_path;    /* -c / --config (required)                      */
    const char *blocks_file;    /* -l / -b / --blocks, NULL = every shapefile ID */
    bool overwrite;             /* -o / --overwrite                              */
    int gpus;                   /* --gpus N, 0 = config key "gpus" or all visible */
    const char *lookups;        /* --lookups g_ii[,..]: overrides the config key "lookups"       */
    const char *conditions;     /* --conditions drained|undrained|both: overrides "conditions" */
    const char *compress;       /* --compress deflate|lzw: overrides the config key "compress"   */
    bool cog;                   /* --cog: Cloud Optimized GeoTIFFs (sets the config key "cog")   */
    const char *overview_resampling;    /* --overview-resampling nearest|average                 */
    bool stats;                 /* --stats: GDAL band statistics in every raster (sets the config key "stats") */
    const char *nodata;         /* --nodata none|0..255: overrides the config key "nodata"                */
    bool verify;                /* --verify: check the rasters that exist instead of writing (sets the config key "verify") */
    bool zonal;                 /* --zonal: composite curve numbers per zone instead of rasters (sets the config key "zonal") */
    const char *zones;          /* --zones <file.shp>: overrides the config key "zones_shp_path" and implies --zonal */
    const char *aggregate;      /* --aggregate <f>: overrides the config key "aggregate" */
    const char *grid;           /* --grid <xmin>,<ymax>,<dx>,<dy>,<nx>,<ny>: overrides the config key "grid" */
    const char *storm;          /* --storm <P>[,<lambda>]: overrides the config key "storm" */
    const char *storms;         /* --storms <P1>[:<P2>...][,<lambda>]: overrides the config key "storms" */
    const char *rain;           /* --rain <file>: overrides the config key "rain" */
    const char *rain_unit;      /* --rain-unit <unit>[,<lambda>]: overrides the config key "rain_unit" */
    const char *zone_rain;      /* --zone-rain <file>: overrides the config key "zone_rain" */
    const char *zone_rain_unit; /* --zone-rain-unit <unit>[,<lambda>]: overrides the config key "zone_rain_unit" */
    const char *rains;          /* --rains <file1>[:<file2>...]: overrides the config key "rains" */
    const char *zone_rains;     /* --zone-rains <file1>[:<file2>...]: overrides the config key "zone_rains" */
    const char *runoff_rain;    /* --runoff-rain <file>: overrides the config key "runoff_rain" */
    const char *runoff_rain_unit;   /* --runoff-rain-unit <unit>[,<lambda>]: overrides the config key "runoff_rain_unit" */
    const char *runoff_unit;    /* --runoff-unit <mm>: overrides the config key "runoff_unit" */
} gcn10_run_options;

/* ------------------------------------------------------------------------ */
/* verification (config key "verify", --verify): no counterpart in the reference                            */
/* ------------------------------------------------------------------------ */

/* What a raster file can have wrong before any pixel is looked at, in the order it is checked. */
enum {
    GCN10_VERIFY_OK = 0,
    GCN10_VERIFY_MISSING = 1,       /* no such file */
    GCN10_VERIFY_NOT_TIFF = 2,      /* not a TIFF the reader opens */
    GCN10_VERIFY_NOT_BYTE = 3,      /* not one band of Byte samples */
    GCN10_VERIFY_SIZE = 4,          /* another size than the block's window */
    GCN10_VERIFY_GEOTRANSFORM = 5,  /* another geotransform than the clipped window's (the six doubles, exactly) */
    GCN10_VERIFY_CHUNK = 6,         /* a tile or strip without bytes, or with bytes beyond the end of the file */
    GCN10_VERIFY_OVERVIEW = 7,      /* an overview directory whose size is not the halving rule's */
    GCN10_VERIFY_DECODE = 8,        /* a tile or strip that does not decode (found with the pixels, not by the check below) */
    GCN10_VERIFY_PIXELS = 9         /* pixels differ (likewise) */
};
/* The structure of one output raster: the checks 1..7 above against the window (xsize x ysize, geotransform gt) of
 * its block.  Returns the first finding (GCN10_VERIFY_OK: none) and its text in `reason`; *n_levels (optional)
 * receives the number of overview directories behind the raster. */
int gcn10_verify_structure(const char *path, int xsize, int ysize, const double gt[6], int *n_levels,
                           char *reason, size_t reason_cap);

/* Runs the whole job: config, logs, block ids, lookup tables, one worker thread
 * per GPU pulling block ids from a shared atomic counter (replaces the static
 * round-robin over MPI ranks, src/main.c:171), per block: windows, index maps,
 * pinned-host strips double-buffered against the fused kernel, 18 tiled DEFLATE
 * GeoTIFFs named as src/cn.c:308, 341.  Returns the process exit code: 0, or 1
 * where the reference calls MPI_Abort(.., 1).  A verify run (opt->verify / "verify=1") writes no raster: 0 = every
 * selected raster of every block verified, 2 = it ran to its end and found a bad or missing file, 1 as above.  A zonal
 * run (opt->zonal / "zonal=1") writes no raster either, only its table: exit codes as for a write run, and 1 as well
 * when a block's inputs could not be read (the table is written, but lacks that block).  An aggregate run
 * (opt->aggregate / "aggregate=<f>") writes cn_rasters_<cond>_x<f>/ instead of the 10 m rasters: exit codes as for a
 * write run.  A grid run (opt->grid / "grid=...") writes cn_grid_<cond>/cn_<hc>_<arc>.tif, one raster per selected
 * raster on the model grid, after the last block: exit codes as for a zonal run (1 as well when a block's inputs could
 * not be read: the rasters are written, but lack that block).  A storm (opt->storm / "storm=<P>[,<lambda>]") adds
 * cn_grid_<cond>/cnq_<hc>_<arc>_p<N>.tif to a grid run and the columns runoff_mm,cn_runoff to a zonal run's table;
 * several storms (opt->storms / "storms=<P1>[:<P2>...][,<lambda>]") add one such raster per storm, or the columns
 * runoff_mm_p<N>,cn_runoff_p<N> per storm (with one depth: exactly what storm adds).  A rainfall raster (opt->rain /
 * "rain=<file>", with opt->rain_unit / "rain_unit=<unit>[,<lambda>]") adds cn_grid_<cond>/cnq_<hc>_<arc>_rain.tif to a
 * grid run, every cell for its own depth; the means are byte for byte those of the run without it.  Several rainfall
 * rasters (opt->rains / "rains=<file1>[:<file2>...]", with the same unit) add cnq_<hc>_<arc>_rain<j>.tif per file to a
 * grid run that counts its pixels once (with one file: exactly what rain adds).  A rainfall raster
 * under the zones (opt->zone_rain / "zone_rain=<file>", with opt->zone_rain_unit / "zone_rain_unit=...") adds the columns
 * rain_pixels,rain_mm,rain_valid,runoff_mm_rain,cn_runoff_rain to a zonal run's table ("A rainfall raster under the
 * zones" above); the other columns are byte for byte those of the run without it.  Several such rasters
 * (opt->zone_rains / "zone_rains=<file1>[:<file2>...]", with the same unit) add rain_pixels,rain_valid and three columns
 * per file to a zonal run that counts its pixels once (with one file: exactly what zone_rain adds). */
int gcn10_run(const gcn10_run_options *opt);

/* Path of the HIP library this process would load (diagnostics). */
const char *gcn10_gpu_library_path(void);

#ifdef __cplusplus
}
#endif
#endif /* GCN10_HOST_H */
