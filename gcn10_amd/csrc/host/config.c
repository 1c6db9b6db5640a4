/* config.c -- key=value run configuration.
 *
 * Same file grammar and the same five required keys as the reference's
 * parse_config() (/root/reference/src/config.c:44-114): '#' comment lines,
 * lines without '=' ignored, unknown keys ignored, surrounding whitespace
 * trimmed, 511-byte lines.  Existing gcn10 config files work unchanged; a few
 * optional keys steer the GPU pipeline.
 */
#include "gcn10_host.h"

#include <ctype.h>
#include <stdbool.h>
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>

static char *strip(char *s)
{
    char *e;

    while (*s && isspace((unsigned char)*s))
        s++;
    e = s + strlen(s);
    while (e > s && isspace((unsigned char)e[-1]))
        e--;
    *e = '\0';
    return s;
}

static int set_str(char **slot, const char *val)
{
    char *copy = strdup(val);

    if (!copy)
        return -1;
    free(*slot);        /* a repeated key: the last one wins, as in the reference */
    *slot = copy;
    return 0;
}

int gcn10_parse_lookups(const char *text, unsigned *mask)
{
    char buf[256];
    unsigned m = 0;

    if (!text || strlen(text) >= sizeof buf)
        return -1;
    strcpy(buf, text);
    for (char *tok = strtok(buf, ", \t"); tok; tok = strtok(NULL, ", \t")) {
        bool found = false;

        if (!strcmp(tok, "all")) {
            m |= 0x1ffu;
            continue;
        }
        for (int hi = 0; hi < 3 && !found; hi++)
            for (int ai = 0; ai < 3 && !found; ai++) {
                char name[16];

                snprintf(name, sizeof name, "%s_%s", gcn10_hcs[hi], gcn10_arcs[ai]);
                if (!strcmp(tok, name)) {
                    m |= 1u << (hi * 3 + ai);
                    found = true;
                }
            }
        if (!found)
            return -1;
    }
    if (!m)
        return -1;
    *mask = m;
    return 0;
}

int gcn10_parse_conditions(const char *text, unsigned *mask)
{
    char buf[64];
    unsigned m = 0;

    if (!text || strlen(text) >= sizeof buf)
        return -1;
    strcpy(buf, text);
    for (char *tok = strtok(buf, ", \t"); tok; tok = strtok(NULL, ", \t")) {
        if (!strcmp(tok, "both") || !strcmp(tok, "all"))
            m |= 3u;
        else if (!strcmp(tok, gcn10_conds[0]))
            m |= 1u;
        else if (!strcmp(tok, gcn10_conds[1]))
            m |= 2u;
        else
            return -1;
    }
    if (!m)
        return -1;
    *mask = m;
    return 0;
}

int gcn10_parse_compress(const char *text, int *codec)
{
    if (!text)
        return -1;
    if (!strcasecmp(text, "deflate"))
        *codec = GCN10_COMPRESS_DEFLATE;
    else if (!strcasecmp(text, "lzw"))
        *codec = GCN10_COMPRESS_LZW;
    else
        return -1;
    return 0;
}

int gcn10_parse_overview_resampling(const char *text, int *method)
{
    if (!text)
        return -1;
    if (!strcasecmp(text, "nearest"))
        *method = GCN10_OVERVIEW_NEAREST;
    else if (!strcasecmp(text, "average"))
        *method = GCN10_OVERVIEW_AVERAGE;
    else
        return -1;
    return 0;
}

int gcn10_parse_cog(const char *text, int *cog)
{
    if (!text || (strcmp(text, "0") != 0 && strcmp(text, "1") != 0))
        return -1;
    *cog = text[0] == '1';
    return 0;
}

int gcn10_parse_stats(const char *text, int *stats)
{
    return gcn10_parse_cog(text, stats);       /* the same "0" | "1" */
}

int gcn10_parse_verify(const char *text, int *verify)
{
    return gcn10_parse_cog(text, verify);      /* the same "0" | "1" */
}

int gcn10_parse_zonal(const char *text, int *zonal)
{
    return gcn10_parse_cog(text, zonal);       /* the same "0" | "1" */
}

int gcn10_parse_aggregate(const char *text, int *factor)
{
    int v = 0;

    if (!text || !*text)
        return -1;
    for (const char *c = text; *c; c++) {
        if (*c < '0' || *c > '9' || c - text >= 3)
            return -1;
        v = v * 10 + (*c - '0');
    }
    if (v != 0 && (v < 2 || v > 256))
        return -1;
    *factor = v;
    return 0;
}

int gcn10_parse_nodata(const char *text, int *nodata)
{
    int v = 0;

    if (!text || !*text)
        return -1;
    if (!strcasecmp(text, "none")) {
        *nodata = -1;
        return 0;
    }
    for (const char *c = text; *c; c++) {
        if (*c < '0' || *c > '9' || c - text >= 3)
            return -1;
        v = v * 10 + (*c - '0');
    }
    if (v > 255)
        return -1;
    *nodata = v;
    return 0;
}

int gcn10_config_parse(const char *path, gcn10_config *cfg, char *err, size_t errcap)
{
    char line[512];                                     /* src/config.c:47 */
    FILE *f;

    memset(cfg, 0, sizeof *cfg);
    cfg->gpu_deflate = 2;
    cfg->gpu_inflate = 1;
    cfg->gpu_inflate_lzw = 1;
    cfg->prefetch_blocks = 1;
    cfg->table_mask = 0x1ffu;
    cfg->cond_mask = 3u;
    cfg->nodata = -1;
    f = fopen(path, "r");
    if (!f) {
        snprintf(err, errcap, "cannot open config '%s'", path);     /* src/config.c:52 */
        return -1;
    }
    while (fgets(line, sizeof line, f)) {
        char *p = strip(line);
        char *eq, *key, *val;
        int rc = 0;

        if (*p == '\0' || *p == '#')
            continue;
        eq = strchr(p, '=');
        if (!eq)
            continue;
        *eq = '\0';
        key = strip(p);
        val = strip(eq + 1);

        if (!strcmp(key, "hysogs_data_path"))
            rc = set_str(&cfg->hysogs_data_path, val);
        else if (!strcmp(key, "esa_data_path"))
            rc = set_str(&cfg->esa_data_path, val);
        else if (!strcmp(key, "blocks_shp_path"))
            rc = set_str(&cfg->blocks_shp_path, val);
        else if (!strcmp(key, "lookup_table_path"))
            rc = set_str(&cfg->lookup_table_path, val);
        else if (!strcmp(key, "log_dir"))
            rc = set_str(&cfg->log_dir, val);
        else if (!strcmp(key, "esa_tile_dir"))
            rc = set_str(&cfg->esa_tile_dir, val);
        else if (!strcmp(key, "gpus"))
            cfg->gpus = atoi(val);
        else if (!strcmp(key, "workers_per_gpu"))
            cfg->workers_per_gpu = atoi(val);
        else if (!strcmp(key, "strip_rows"))
            cfg->strip_rows = atoi(val);
        else if (!strcmp(key, "gpu_inflate"))
            cfg->gpu_inflate = atoi(val) != 0;
        else if (!strcmp(key, "gpu_inflate_lzw"))
            cfg->gpu_inflate_lzw = atoi(val) != 0;
        else if (!strcmp(key, "io_threads"))
            cfg->io_threads = atoi(val);
        else if (!strcmp(key, "direct_io"))
            cfg->direct_io = atoi(val) != 0;
        else if (!strcmp(key, "prefetch_blocks"))
            cfg->prefetch_blocks = atoi(val) != 0;
        else if (!strcmp(key, "deflate_level"))
            cfg->deflate_level = atoi(val);
        else if (!strcmp(key, "gpu_deflate"))
            cfg->gpu_deflate = atoi(val) < 0 ? 0 : (atoi(val) > 2 ? 2 : atoi(val));
        else if (!strcmp(key, "lookups") || !strcmp(key, "conditions")) {
            const bool lk = key[0] == 'l';

            if ((lk ? gcn10_parse_lookups(val, &cfg->table_mask) : gcn10_parse_conditions(val, &cfg->cond_mask)) != 0) {
                fclose(f);
                snprintf(err, errcap, "bad value for %s: '%s' (%s)", key, val,
                         lk ? "names like g_ii, p_i,f_iii or all" : "drained, undrained or both");
                gcn10_config_free(cfg);
                return -3;
            }
        }
        else if (!strcmp(key, "compress") && gcn10_parse_compress(val, &cfg->compress) != 0) {
            fclose(f);
            snprintf(err, errcap, "bad value for compress: '%s' (deflate or lzw)", val);
            gcn10_config_free(cfg);
            return -3;
        }
        else if (!strcmp(key, "cog") && gcn10_parse_cog(val, &cfg->cog) != 0) {
            fclose(f);
            snprintf(err, errcap, "bad value for cog: '%s' (0 or 1)", val);
            gcn10_config_free(cfg);
            return -3;
        }
        else if (!strcmp(key, "overview_resampling") &&
                 gcn10_parse_overview_resampling(val, &cfg->overview_resampling) != 0) {
            fclose(f);
            snprintf(err, errcap, "bad value for overview_resampling: '%s' (nearest or average)", val);
            gcn10_config_free(cfg);
            return -3;
        }
        else if (!strcmp(key, "stats") && gcn10_parse_stats(val, &cfg->stats) != 0) {
            fclose(f);
            snprintf(err, errcap, "bad value for stats: '%s' (0 or 1)", val);
            gcn10_config_free(cfg);
            return -3;
        }
        else if (!strcmp(key, "nodata") && gcn10_parse_nodata(val, &cfg->nodata) != 0) {
            fclose(f);
            snprintf(err, errcap, "bad value for nodata: '%s' (none or an integer 0..255)", val);
            gcn10_config_free(cfg);
            return -3;
        }
        else if (!strcmp(key, "verify") && gcn10_parse_verify(val, &cfg->verify) != 0) {
            fclose(f);
            snprintf(err, errcap, "bad value for verify: '%s' (0 or 1)", val);
            gcn10_config_free(cfg);
            return -3;
        }
        else if (!strcmp(key, "zonal") && gcn10_parse_zonal(val, &cfg->zonal) != 0) {
            fclose(f);
            snprintf(err, errcap, "bad value for zonal: '%s' (0 or 1)", val);
            gcn10_config_free(cfg);
            return -3;
        }
        else if (!strcmp(key, "aggregate") && gcn10_parse_aggregate(val, &cfg->aggregate) != 0) {
            fclose(f);
            snprintf(err, errcap, "bad value for aggregate: '%s' (0 or an integer 2..256)", val);
            gcn10_config_free(cfg);
            return -3;
        }
        else if (!strcmp(key, "grid")) {
            gcn10_grid g;

            if (gcn10_parse_grid(val, &g) != 0) {
                fclose(f);
                snprintf(err, errcap, "bad value for grid: '%s' (xmin,ymax,dx,dy,nx,ny)", val);
                gcn10_config_free(cfg);
                return -3;
            }
            rc = set_str(&cfg->grid, val);
        }
        else if (!strcmp(key, "storm")) {
            if (gcn10_parse_storm(val, &cfg->storm_p, &cfg->storm_lambda) != 0) {
                fclose(f);
                snprintf(err, errcap, "bad value for storm: '%s' (P[,lambda]: 0 < P <= 650 mm, 0 <= lambda < 1)", val);
                gcn10_config_free(cfg);
                return -3;
            }
            rc = set_str(&cfg->storm, val);
        }
        else if (!strcmp(key, "storms")) {
            if (gcn10_parse_storms(val, cfg->storms_p, &cfg->n_storms, &cfg->storms_lambda) != 0) {
                fclose(f);
                snprintf(err, errcap, "bad value for storms: '%s' (P1[:P2...][,lambda]: 1 to 8 rising depths, 0 < P <= 650 "
                                      "mm, 0 <= lambda < 1)", val);
                gcn10_config_free(cfg);
                return -3;
            }
            rc = set_str(&cfg->storms, val);
        }
        else if (!strcmp(key, "rain"))
            rc = set_str(&cfg->rain, val);
        else if (!strcmp(key, "rain_unit")) {
            double unit, lambda;

            if (gcn10_parse_rain_unit(val, &unit, &lambda) != 0) {
                fclose(f);
                snprintf(err, errcap, "bad value for rain_unit: '%s' (unit[,lambda]: 0 < unit, 255 unit <= 650 mm, 0 <= "
                                      "lambda < 1)", val);
                gcn10_config_free(cfg);
                return -3;
            }
            rc = set_str(&cfg->rain_unit, val);
        }
        else if (!strcmp(key, "rains"))
            rc = set_str(&cfg->rains, val);
        else if (!strcmp(key, "zone_rain"))
            rc = set_str(&cfg->zone_rain, val);
        else if (!strcmp(key, "zone_rains"))
            rc = set_str(&cfg->zone_rains, val);
        else if (!strcmp(key, "zone_rain_unit")) {
            double unit, lambda;

            if (gcn10_parse_rain_unit(val, &unit, &lambda) != 0) {
                fclose(f);
                snprintf(err, errcap, "bad value for zone_rain_unit: '%s' (unit[,lambda]: 0 < unit, 255 unit <= 650 mm, "
                                      "0 <= lambda < 1)", val);
                gcn10_config_free(cfg);
                return -3;
            }
            rc = set_str(&cfg->zone_rain_unit, val);
        }
        else if (!strcmp(key, "runoff_rain"))
            rc = set_str(&cfg->runoff_rain, val);
        else if (!strcmp(key, "runoff_rain_unit")) {
            double unit, lambda;

            if (gcn10_parse_rain_unit(val, &unit, &lambda) != 0) {
                fclose(f);
                snprintf(err, errcap, "bad value for runoff_rain_unit: '%s' (unit[,lambda]: 0 < unit, 255 unit <= 650 mm, "
                                      "0 <= lambda < 1)", val);
                gcn10_config_free(cfg);
                return -3;
            }
            rc = set_str(&cfg->runoff_rain_unit, val);
        }
        else if (!strcmp(key, "runoff_unit")) {
            unsigned u;

            if (gcn10_parse_runoff_unit(val, &u) != 0) {
                fclose(f);
                snprintf(err, errcap, "bad value for runoff_unit: '%s' (millimetres per count, 0.01 to 650)", val);
                gcn10_config_free(cfg);
                return -3;
            }
            rc = set_str(&cfg->runoff_unit, val);
        }
        else if (!strcmp(key, "zones_shp_path"))
            rc = set_str(&cfg->zones_shp_path, val);
        else if (!strcmp(key, "zonal_output"))
            rc = set_str(&cfg->zonal_output, val);
        else if (!strcmp(key, "zones_id_field")) {
            if (!*val || strlen(val) > 10) {        /* a dBASE field name has at most 10 characters */
                fclose(f);
                snprintf(err, errcap, "bad value for zones_id_field: '%s' (a .dbf field name, 1..10 characters)", val);
                gcn10_config_free(cfg);
                return -3;
            }
            rc = set_str(&cfg->zones_id_field, val);
        }
        if (rc != 0) {
            fclose(f);
            snprintf(err, errcap, "malloc failed for %s", key);     /* src/config.c:71 */
            gcn10_config_free(cfg);
            return -1;
        }
    }
    fclose(f);
    if (cfg->compress == GCN10_COMPRESS_LZW && cfg->gpu_deflate == 0) {
        snprintf(err, errcap, "bad value for compress: 'lzw' with gpu_deflate=0 (LZW tiles are encoded on the GPU "
                              "only; there is no host LZW encoder)");
        gcn10_config_free(cfg);
        return -3;
    }
    if (cfg->cog && cfg->gpu_deflate == 0) {
        snprintf(err, errcap, "bad value for cog: '1' with gpu_deflate=0 (overviews are built and encoded on the GPU "
                              "only; there is no host fallback)");
        gcn10_config_free(cfg);
        return -3;
    }

    if (!cfg->hysogs_data_path || !cfg->esa_data_path || !cfg->blocks_shp_path ||
        !cfg->lookup_table_path || !cfg->log_dir) {
        snprintf(err, errcap,                                       /* src/config.c:109-111 */
                 "missing one of: hysogs_data_path, esa_data_path,\n"
                 "blocks_shp_path, lookup_table_path, log_dir");
        gcn10_config_free(cfg);
        return -2;
    }
    return 0;
}

void gcn10_config_free(gcn10_config *cfg)
{
    free(cfg->hysogs_data_path);
    free(cfg->esa_data_path);
    free(cfg->blocks_shp_path);
    free(cfg->lookup_table_path);
    free(cfg->log_dir);
    free(cfg->esa_tile_dir);
    free(cfg->zones_shp_path);
    free(cfg->zones_id_field);
    free(cfg->zonal_output);
    free(cfg->grid);
    free(cfg->storm);
    free(cfg->storms);
    free(cfg->rain);
    free(cfg->rain_unit);
    free(cfg->zone_rain);
    free(cfg->zone_rain_unit);
    free(cfg->rains);
    free(cfg->zone_rains);
    free(cfg->runoff_rain);
    free(cfg->runoff_rain_unit);
    free(cfg->runoff_unit);
    memset(cfg, 0, sizeof *cfg);
}
