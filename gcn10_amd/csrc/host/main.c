/* main.c -- the gcn10 command line.
 *
 * Same flags as the reference program (/root/reference/src/main.c:85-98):
 *   gcn10 -c|--config <file> [-l|--blocks <file>] [-o|--overwrite] [-h|--help] [-v|--version]
 * plus -b as a synonym of -l (the reference's usage text advertises -b,
 * src/main.c:28, while its parser only takes -l, src/main.c:90), --gpus N, and --lookups /
 * --conditions to produce a subset of the 18 rasters (BASELINE config 3: "single lookup"), and --compress to
 * write LZW instead of DEFLATE GeoTIFFs, --stats / --nodata for GDAL band statistics and a NoData tag, and --verify
 * to check the rasters a run has written instead of writing them, and --zonal / --zones for the composite curve
 * numbers of the polygons of a shapefile instead of rasters, and --aggregate for area-mean rasters on a coarser grid,
 * and --grid for mean rasters on a model grid that spans the blocks, and --storm for the runoff-weighted composites of
 * a design storm beside the means of --grid and --zones, and --storms for a ladder of such storms in one run.
 * No mpirun: one process drives every GPU of the node.
 */
#include "gcn10_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static void usage(FILE *fp)
{
    fprintf(fp,
            "gcn10 - high-resolution curve number generator, MI355X edition\n"
            "usage:\n"
            "  gcn10 --config <config.txt> [--blocks <blocks.txt>] [--overwrite] [--gpus <n>]\n"
            "        [--lookups <names>] [--conditions drained|undrained|both] [--compress deflate|lzw]\n"
            "        [--cog] [--overview-resampling nearest|average] [--stats] [--nodata none|<0..255>]\n"
            "        [--verify] [--zonal] [--zones <zones.shp>] [--aggregate <f>]\n"
            "        [--grid <xmin>,<ymax>,<dx>,<dy>,<nx>,<ny>] [--storm <P>[,<lambda>]]\n"
            "        [--storms <P1>[:<P2>...][,<lambda>]] [--rain <file> [--rain-unit <unit>[,<lambda>]]]\n"
            "        [--rains <file1>[:<file2>...]] [--zone-rain <file> [--zone-rain-unit <unit>[,<lambda>]]]\n"
            "        [--zone-rains <file1>[:<file2>...]]\n"
            "  gcn10 --help | -h | --version | -v\n"
            "\n"
            "options:\n"
            "  --config, -c <file>\tpath to config file (required)\n"
            "  --blocks, -l, -b <file>\toptional list of block ids to process\n"
            "  --overwrite, -o\toverwrite existing outputs if present (optional)\n"
            "  --gpus <n>\t\tnumber of GPUs to use (default: all visible)\n"
            "  --lookups <names>\tonly these lookups, e.g. g_ii or p_i,f_iii (default: all nine)\n"
            "  --conditions <c>\tdrained, undrained or both (default: both)\n"
            "  --compress <c>\tdeflate or lzw: compression of the GeoTIFFs (default: deflate)\n"
            "  --cog\t\t\tCloud Optimized GeoTIFFs with overviews built on the GPU (config key cog=1)\n"
            "  --overview-resampling <m>\tnearest or average: how the overviews are made (default: nearest)\n"
            "  --stats\t\tGDAL band statistics in every raster, counted on the GPU (config key stats=1)\n"
            "  --nodata <v>\t\tnone or 0..255: declare that NoData value, left out of the statistics (default: none)\n"
            "  --verify\t\twrite nothing: decode the rasters that exist on the GPU and compare every pixel with\n"
            "\t\t\tthe value computed now (config key verify=1); exit code 2 = a bad or missing raster,\n"
            "\t\t\ttheir blocks listed in <log_dir>/verify_failed_blocks.txt; not with --overwrite\n"
            "  --zonal\t\twrite no raster but one table, zonal_cn.csv (config key zonal_output): the composite\n"
            "\t\t\t(pixel-weighted mean) curve number of every polygon of zones_shp_path and every selected\n"
            "\t\t\traster, counted on the GPU (config key zonal=1); not with --overwrite or --verify\n"
            "  --zones <file.shp>\tthe zone polygons, in the landcover's CRS (config key zones_shp_path; the zone id\n"
            "\t\t\tis the numeric field zones_id_field, default ID); implies --zonal\n"
            "  --aggregate <f>\twrite no 10 m raster but, under cn_rasters_<cond>_x<f>/, the mean of every selected\n"
            "\t\t\traster over cells of f x f landcover pixels (f = 2..256), reduced on the GPU (config key\n"
            "\t\t\taggregate=<f>); not with --verify or --zonal\n"
            "  --grid <xmin>,<ymax>,<dx>,<dy>,<nx>,<ny>\n"
            "\t\t\twrite no 10 m raster but, under cn_grid_<cond>/, ONE raster per selected raster on a\n"
            "\t\t\tmodel grid in the landcover's CRS: nx x ny cells of dx x dy units (8 landcover pixels or\n"
            "\t\t\tmore) from the upper-left corner (xmin, ymax), each the mean over its pixels of all\n"
            "\t\t\tprocessed blocks, reduced on the GPU (config key grid=...); not with --verify, --zonal,\n"
            "\t\t\t--aggregate, --overwrite or --compress lzw\n"
            "  --storm <P>[,<lambda>]\ta design storm: P mm of rain (0 < P <= 650) and the initial-abstraction ratio\n"
            "\t\t\t(0 <= lambda < 1, default 0.2).  With --grid, a second raster per selected raster,\n"
            "\t\t\tcn_grid_<cond>/cnq_<hc>_<arc>_p<100 P>.tif: the runoff-equivalent CN of every cell, the\n"
            "\t\t\tcurve number that yields the cell's mean runoff depth for that storm, summed on the GPU;\n"
            "\t\t\twith --zones, the columns runoff_mm,cn_runoff (config key storm=...); needs --grid or\n"
            "\t\t\t--zones, not with --aggregate or --verify\n"
            "  --storms <P1>[:<P2>...][,<lambda>]\n"
            "\t\t\t1 to 8 design storms of rising depth and one ratio in ONE run: every block is read,\n"
            "\t\t\tdecoded and summed once.  With --grid, cnq_<hc>_<arc>_p<100 P_k>.tif per storm, each the\n"
            "\t\t\tfile --storm <P_k>,<lambda> alone writes; with --zones, the columns runoff_mm_p<100 P_k>,\n"
            "\t\t\tcn_runoff_p<100 P_k> per storm (one depth: exactly what --storm gives; config key\n"
            "\t\t\tstorms=...); not with --storm, otherwise as --storm\n"
            "  --rain <file>\t\ta rainfall raster on the model grid: a one-band Byte GeoTIFF of nx x ny pixels, a cell\n"
            "\t\t\twith byte b has P = b x unit mm of rain (every byte is a depth, 0 = no rain).  With --grid,\n"
            "\t\t\tcn_grid_<cond>/cnq_<hc>_<arc>_rain.tif beside every mean: the runoff-equivalent CN of every\n"
            "\t\t\tcell for the cell's own depth, summed on the GPU (config key rain=...); needs --grid, not\n"
            "\t\t\twith --storm, --storms, --zonal, --aggregate or --verify\n"
            "  --rain-unit <unit>[,<lambda>]\n"
            "\t\t\tmillimetres per count of --rain (0 < unit, 255 unit <= 650, default 1) and the\n"
            "\t\t\tinitial-abstraction ratio (0 <= lambda < 1, default 0.2; config key rain_unit=...)\n"
            "  --rains <file1>[:<file2>...]\n"
            "\t\t\t1 to 8 rainfall rasters as --rain takes one, in ONE run: every block is read, decoded\n"
            "\t\t\tand counted once.  cnq_<hc>_<arc>_rain<j>.tif per file, each the file --rain <file_j>\n"
            "\t\t\talone writes (one file: exactly what --rain gives; config key rains=...); --rain-unit\n"
            "\t\t\tholds for all files; not with --rain, otherwise as --rain\n"
            "  --zone-rain <file>\ta rainfall raster under the zones: a one-band Byte GeoTIFF with its own geotransform\n"
            "\t\t\t(north up, the landcover's CRS), byte b = b x unit mm of rain.  With --zones, the columns\n"
            "\t\t\train_pixels,rain_mm,rain_valid,runoff_mm_rain,cn_runoff_rain: every zone's runoff under\n"
            "\t\t\tthe field, reduced on the GPU, and the CN that yields it with the zone's mean depth\n"
            "\t\t\t(config key zone_rain=...); needs --zones, not with --storm or --storms\n"
            "  --zone-rain-unit <unit>[,<lambda>]\n"
            "\t\t\tas --rain-unit, for --zone-rain and --zone-rains (config key zone_rain_unit=...)\n"
            "  --zone-rains <file1>[:<file2>...]\n"
            "\t\t\t1 to 8 rainfall rasters as --zone-rain takes one, on one grid, in ONE run: every block\n"
            "\t\t\tis read, decoded, scan-converted and counted once.  rain_pixels,rain_valid, then\n"
            "\t\t\train_mm_rain<j>,runoff_mm_rain<j>,cn_runoff_rain<j> per file, each what --zone-rain\n"
            "\t\t\t<file_j> alone prints (one file: exactly the table of --zone-rain; config key\n"
            "\t\t\tzone_rains=...); not with --zone-rain, otherwise as --zone-rain\n"
            "  --runoff-rain <file>\twrite, instead of the curve numbers, the runoff depth of every 10 m pixel under a\n"
            "\t\t\trainfall raster (one Byte band with a geotransform, as --zone-rain takes it):\n"
            "\t\t\trunoff_rasters_<cond>/q_<hc>_<arc>_<id>.tif, 255 = no value or no rain cell (config key\n"
            "\t\t\trunoff_rain=...); not with --verify, --aggregate, --zones, --grid, --storm(s), --rain(s),\n"
            "\t\t\t--zone-rain(s), --cog or --stats\n"
            "  --runoff-rain-unit <unit>[,<lambda>]\n"
            "\t\t\tas --rain-unit, for --runoff-rain (config key runoff_rain_unit=...)\n"
            "  --runoff-unit <mm>\tmillimetres per count of the written rasters, 0.01 to 650 (default: the rain unit;\n"
            "\t\t\tconfig key runoff_unit=...)\n"
            "  --help, -h\t\tshow this help and exit\n"
            "  --version, -v\tprint version and exit\n"
            "\n"
            "notes:\n"
            "  one process drives all GPUs of the node; 'mpirun -n <ranks>' is not needed.\n"
            "  outputs go to ./cn_rasters_drained and ./cn_rasters_undrained.\n");
}

int main(int argc, char **argv)
{
    gcn10_run_options opt;

    /* --help / --version before anything else (src/main.c:39-56, 66-69) */
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--help") || !strcmp(argv[i], "-h")) {
            usage(stdout);
            return 0;
        }
        if (!strcmp(argv[i], "--version") || !strcmp(argv[i], "-v")) {
            printf("gcn10 %s\n", GCN10_VERSION);
            return 0;
        }
    }
    memset(&opt, 0, sizeof opt);
    for (int i = 1; i < argc; i++) {            /* src/main.c:85-98 */
        if ((!strcmp(argv[i], "-c") || !strcmp(argv[i], "--config")) && i + 1 < argc)
            opt.config_path = argv[++i];
        else if ((!strcmp(argv[i], "-l") || !strcmp(argv[i], "-b") || !strcmp(argv[i], "--blocks")) &&
                 i + 1 < argc)
            opt.blocks_file = argv[++i];
        else if (!strcmp(argv[i], "-o") || !strcmp(argv[i], "--overwrite"))
            opt.overwrite = true;
        else if (!strcmp(argv[i], "--gpus") && i + 1 < argc)
            opt.gpus = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--lookups") && i + 1 < argc)
            opt.lookups = argv[++i];
        else if (!strcmp(argv[i], "--conditions") && i + 1 < argc)
            opt.conditions = argv[++i];
        else if (!strcmp(argv[i], "--compress") && i + 1 < argc)
            opt.compress = argv[++i];
        else if (!strcmp(argv[i], "--cog"))
            opt.cog = true;
        else if (!strcmp(argv[i], "--overview-resampling") && i + 1 < argc)
            opt.overview_resampling = argv[++i];
        else if (!strcmp(argv[i], "--stats"))
            opt.stats = true;
        else if (!strcmp(argv[i], "--nodata") && i + 1 < argc)
            opt.nodata = argv[++i];
        else if (!strcmp(argv[i], "--verify"))
            opt.verify = true;
        else if (!strcmp(argv[i], "--aggregate") && i + 1 < argc)
            opt.aggregate = argv[++i];
        else if (!strcmp(argv[i], "--grid") && i + 1 < argc)
            opt.grid = argv[++i];
        else if (!strcmp(argv[i], "--storm") && i + 1 < argc)
            opt.storm = argv[++i];
        else if (!strcmp(argv[i], "--storms") && i + 1 < argc)
            opt.storms = argv[++i];
        else if (!strcmp(argv[i], "--rain") && i + 1 < argc)
            opt.rain = argv[++i];
        else if (!strcmp(argv[i], "--rain-unit") && i + 1 < argc)
            opt.rain_unit = argv[++i];
        else if (!strcmp(argv[i], "--rains") && i + 1 < argc)
            opt.rains = argv[++i];
        else if (!strcmp(argv[i], "--zone-rain") && i + 1 < argc)
            opt.zone_rain = argv[++i];
        else if (!strcmp(argv[i], "--zone-rains") && i + 1 < argc)
            opt.zone_rains = argv[++i];
        else if (!strcmp(argv[i], "--zone-rain-unit") && i + 1 < argc)
            opt.zone_rain_unit = argv[++i];
        else if (!strcmp(argv[i], "--runoff-rain") && i + 1 < argc)
            opt.runoff_rain = argv[++i];
        else if (!strcmp(argv[i], "--runoff-rain-unit") && i + 1 < argc)
            opt.runoff_rain_unit = argv[++i];
        else if (!strcmp(argv[i], "--runoff-unit") && i + 1 < argc)
            opt.runoff_unit = argv[++i];
        else if (!strcmp(argv[i], "--zonal"))
            opt.zonal = true;
        else if (!strcmp(argv[i], "--zones") && i + 1 < argc) {
            opt.zones = argv[++i];
            opt.zonal = true;
        }
    }
    return gcn10_run(&opt);
}
