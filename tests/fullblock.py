"""Full-size blocks end to end: a world of the real VRT geometry, an independent reference of every pixel of the
18 rasters, the model of the two overview resamplings, and a comparator that locates the first wrong pixel.

The world (make_world): esa.vrt over 2 x 2 landcover GeoTIFFs of 36000^2 pixels (1024^2 DEFLATE tiles, 3 x 3
degrees each, the real pixel size), LZW soil 25 times coarser, and three blocks: A on one file whose last
column and row come from its neighbours, B across all four files at an offset that is no multiple of 1024, and a
small C over the corner where the four files meet.

The reference (value_table, block_keys, expected_rows) comes from the oracle alone: the soil row and column
maps of oracle_index_maps, and an 18 x 256 x 256 table of oracle_process_block_mem over every (landcover, soil
code) pair; a pixel of raster r is T[r][landcover, soil code]."""
import math
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from PIL import Image

from oracle import cn_oracle_c as oc
from tests import tiffutil
from tests.util import ESA_CLASSES, HSG_CODES

Image.MAX_IMAGE_PIXELS = None
CONDS, HCS, ARCS = ("drained", "undrained"), ("p", "f", "g"), ("i", "ii", "iii")
DEFAULT_STRIP_ROWS = 2304           # the program's default strip height (pipeline_internal.h)
TILE = 256
THREADS = min(16, len(os.sched_getaffinity(0)))

PX = 8.3333333333330430e-05         # the shipped VRT's pixel size: 36000 px are a hair short of 3 degrees
FILE_PX = 36000
VRT_PX = 2 * FILE_PX
VRT_GT = [0.0, PX, 0.0, 3.0, 0.0, -PX]
SOIL_PX = VRT_PX // 25
SOIL_GT = [0.0, 6.0 / SOIL_PX, 0.0, 3.0, 0.0, -6.0 / SOIL_PX]
# (id, minx, miny, maxx, maxy) in the VRT's coordinates: lon 0 .. 6, lat -3 .. 3
BLOCKS = [(1, 0.0, 0.0, 3.0, 3.0),          # A: the north-west file, plus a column and a row of its neighbours
          (2, 1.7, -1.3, 4.7, 1.7),         # B: all four files, offset (20400, 15600) px
          (3, 2.98, -0.02, 3.03, 0.015)]    # C: 600 x 420 px over the corner where the four files meet
# regions several tiles wide whose tiles are equal in all 18 rasters: (row0, row1, col0, col1, class) in VRT pixels
FLAT = [(8000, 9800, 5000, 7500, 80),       # lake in A
        (4000, 5200, 30000, 33000, 0),      # NoData in A, across the strip boundary at row 4608
        (35000, 37500, 38000, 41000, 80),   # lake in B, across the files' boundary at row 36000
        (48000, 50500, 22000, 25000, 0)]    # NoData in B
DUAL_FREE_LON = 2.5                 # west of it the soil has no dual classes: drained == undrained there


def raster_name(r, bid):
    c, k = divmod(r, 9)
    return os.path.join("cn_rasters_%s" % CONDS[c], "cn_%s_%s_%d.tif" % (HCS[k // 3], ARCS[k % 3], bid))


# ---- the world -------------------------------------------------------------------------------------------------

def make_world(wd, seed=7):
    """Writes tiles/T_<i><j>.tif, esa.vrt, soil.tif and blocks.shp under wd; returns (landcover of the whole VRT,
    soil).  The landcover: bench's "natural" texture per file (its own seed), the FLAT regions, and 0.5 % random
    pixels everywhere (classes {0, 80} inside FLAT, so those tiles stay equal in all rasters), so that no two 256^2
    tiles of a block are equal."""
    import bench
    esa = np.empty((VRT_PX, VRT_PX), np.uint8)
    for i in range(2):
        for j in range(2):
            esa[j * FILE_PX:(j + 1) * FILE_PX, i * FILE_PX:(i + 1) * FILE_PX] = \
                bench.synth_block(seed * 10 + 2 * j + i, FILE_PX, "natural")[0]
    for r0, r1, c0, c1, cls in FLAT:
        esa[r0:r1, c0:c1] = cls
    rng = np.random.default_rng(seed)
    n = VRT_PX * VRT_PX // 200
    idx = rng.integers(0, VRT_PX * VRT_PX, n, dtype=np.int64)
    esa.reshape(-1)[idx] = rng.choice(ESA_CLASSES, n)
    for r0, r1, c0, c1, cls in FLAT:
        sub = esa[r0:r1, c0:c1]
        sub[sub != cls] = 80 - cls
    del idx
    soil = rng.choice(HSG_CODES, size=(SOIL_PX, SOIL_PX)).astype(np.uint8)
    west = soil[:, :int(DUAL_FREE_LON / SOIL_GT[1])]
    west[(west >= 11) & (west <= 14)] -= 10

    os.makedirs(os.path.join(wd, "tiles"), exist_ok=True)
    src = ""
    for j in range(2):
        for i in range(2):
            name = "T_%d%d.tif" % (j, i)
            gt = [i * FILE_PX * PX, PX, 0.0, 3.0 - j * FILE_PX * PX, 0.0, -PX]
            tiffutil.write_tiff(os.path.join(wd, "tiles", name),
                                esa[j * FILE_PX:(j + 1) * FILE_PX, i * FILE_PX:(i + 1) * FILE_PX], gt=gt,
                                compression=8, tile=(1024, 1024), zlevel=1)
            src += ('<ComplexSource resampling="nearest"><SourceFilename relativeToVRT="0">/vsicurl/https://example.'
                    'invalid/map/%s</SourceFilename><SourceBand>1</SourceBand><SrcRect xOff="0" yOff="0" xSize="%d" '
                    'ySize="%d" /><DstRect xOff="%d" yOff="%d" xSize="%d" ySize="%d" /><NODATA>0</NODATA>'
                    '</ComplexSource>\n' % (name, FILE_PX, FILE_PX, i * FILE_PX, j * FILE_PX, FILE_PX, FILE_PX))
    with open(os.path.join(wd, "esa.vrt"), "w") as f:
        f.write('<VRTDataset rasterXSize="%d" rasterYSize="%d">\n<GeoTransform> %r, %r, 0.0, %r, 0.0, %r'
                '</GeoTransform>\n<VRTRasterBand dataType="Byte" band="1"><NoDataValue>0</NoDataValue>\n%s'
                '</VRTRasterBand></VRTDataset>\n' % (VRT_PX, VRT_PX, VRT_GT[0], VRT_GT[1], VRT_GT[3], VRT_GT[5], src))
    tiffutil.write_tiff(os.path.join(wd, "soil.tif"), soil, gt=SOIL_GT, compression=5, rows_per_strip=16)
    tiffutil.write_block_shapefile(os.path.join(wd, "blocks"), BLOCKS)
    return esa, soil


def write_config(wd, run_dir, lookups, **keys):
    """config.txt in run_dir for the world in wd, with the program's defaults except `keys`."""
    lines = dict(hysogs_data_path=os.path.join(wd, "soil.tif"), esa_data_path=os.path.join(wd, "esa.vrt"),
                 esa_tile_dir=os.path.join(wd, "tiles"), blocks_shp_path=os.path.join(wd, "blocks.shp"),
                 lookup_table_path=lookups, log_dir=os.path.join(run_dir, "logs"))
    lines.update({k: str(v) for k, v in keys.items()})
    os.makedirs(run_dir, exist_ok=True)
    with open(os.path.join(run_dir, "config.txt"), "w") as f:
        f.write("".join("%s=%s\n" % kv for kv in lines.items()))


# ---- the reference ---------------------------------------------------------------------------------------------

def value_table(tables) -> np.ndarray:
    """uint8[18, 256, 256]: T[r][landcover class, soil code], from one oracle block over all 65 536 pairs
    (landcover = row, soil = column // 8)."""
    esa = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 2048, axis=1)
    coarse = np.arange(256, dtype=np.uint8)[None, :]
    gt = [0.0, 1.0, 0.0, 0.0, 0.0, -1.0]
    sgt = [4.0, 8.0, 0.0, 0.0, 0.0, -1.0]
    ci, cj = oc.index_maps(gt, sgt, 2048, 256, 256, 1)
    assert (ci[::8] == np.arange(256)).all() and (cj == 0).all()
    return np.ascontiguousarray(oc.process_block_mem(esa, gt, coarse, sgt, tables)[:, :, ::8])


def block_keys(esa, gt, coarse, soil_gt, threads=THREADS) -> np.ndarray:
    """uint16[H, W]: landcover << 8 | soil code of every pixel of a block (esa: the block's landcover window, gt its
    geotransform, coarse the soil window), the soil code by the oracle's index maps."""
    H, W = esa.shape
    ci, cj = oc.index_maps(gt, soil_gt, W, H, coarse.shape[1], coarse.shape[0])
    key = np.empty((H, W), np.uint16)

    def band(y0):
        y1 = min(H, y0 + 512)
        k = key[y0:y1]
        np.left_shift(esa[y0:y1], 8, out=k, dtype=np.uint16)
        k |= coarse[cj[y0:y1]][:, ci]

    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(band, range(0, H, 512)))
    return key


def expected_rows(T, key, r) -> np.ndarray:
    """Raster r where key holds the pixels' (landcover, soil code) pairs."""
    return T[r].reshape(-1)[key]


def key_histogram(key, threads=THREADS) -> np.ndarray:
    """int64[65536]: how often every (landcover, soil code) pair occurs."""
    def band(y0):
        return np.bincount(key[y0:y0 + 1024].reshape(-1), minlength=65536)

    with ThreadPoolExecutor(threads) as ex:
        return sum(ex.map(band, range(0, key.shape[0], 1024)))


def raster_histogram(T, khist, r) -> np.ndarray:
    """int64[256]: the histogram of raster r from the pair histogram."""
    return np.bincount(T[r].reshape(-1), weights=khist, minlength=256).astype(np.int64)


# ---- the model of the two overview resamplings ("Cloud Optimized GeoTIFF output") -------------------

def nearest_level(full, k):
    H, W = full.shape
    ys = np.minimum((np.arange(math.ceil(H / 2 ** k)) << k) + (1 << (k - 1)), H - 1)
    xs = np.minimum((np.arange(math.ceil(W / 2 ** k)) << k) + (1 << (k - 1)), W - 1)
    return full[np.ix_(ys, xs)]


def _average_once(cur):
    h, w = cur.shape
    p = np.full((h + h % 2, w + w % 2), 255, np.int32)      # clipped footprint = padding left out like 255
    p[:h, :w] = cur
    q = p.reshape(p.shape[0] // 2, 2, p.shape[1] // 2, 2)
    valid = q != 255
    s = np.where(valid, q, 0).sum(axis=(1, 3))
    n = valid.sum(axis=(1, 3))
    return np.where(n == 0, 255, (2 * s + n) // np.maximum(2 * n, 1)).astype(np.uint8)


def average_levels(full, L, band=4096):
    """Levels 1 .. L of `average`: every level halves the one above, each output the round-half-up mean of the
    non-255 pixels of its 2 x 2 footprint (255 when there are none).  Computed in bands of rows, a multiple of 2^L
    high, so that full-size rasters fit: every level's rows of one band depend on that band alone."""
    out = [[] for _k in range(L)]
    step = max(band // (1 << L), 1) << L
    for y0 in range(0, full.shape[0], step):
        cur = full[y0:y0 + step]
        for k in range(L):
            cur = _average_once(cur)
            out[k].append(cur)
    return [np.concatenate(o) if o else np.zeros((0, full.shape[1]), np.uint8) for o in out]


# ---- the comparator --------------------------------------------------------------------------------------------

class Mismatch(AssertionError):
    """The first wrong pixel: where it is (block, raster, level, row, column, strip, 256^2 tile) and got / want."""

    def __init__(self, block, raster, level, row, col, got, want, strip_rows, path=""):
        self.block, self.raster, self.level, self.row, self.col = block, raster, level, row, col
        self.got, self.want = got, want
        self.strip = (row << level) // strip_rows
        self.tile = (row // TILE, col // TILE)
        super().__init__("block %s raster %d level %d: first mismatch at row %d col %d: got %d want %d (strip %d of "
                         "%d rows, tile row %d col %d) %s" % (block, raster, level, row, col, got, want, self.strip,
                                                               strip_rows, self.tile[0], self.tile[1], path))


def compare(got, want, block, raster, y0=0, level=0, strip_rows=DEFAULT_STRIP_ROWS, path=""):
    """got, want: rows y0 .. of one raster (at one overview level).  Raises Mismatch on the first difference."""
    if got.shape != want.shape:
        raise AssertionError("block %s raster %d level %d rows from %d: shape %s, want %s %s"
                             % (block, raster, level, y0, got.shape, want.shape, path))
    bad = got != want
    if bad.any():
        y, x = divmod(int(np.argmax(bad.reshape(-1))), want.shape[1])
        raise Mismatch(block, raster, level, y0 + y, x, int(got[y, x]), int(want[y, x]), strip_rows, path)


def decode_levels(path, n_levels):
    """Every level of a GeoTIFF through PIL (libtiff): [full resolution, level 1, ...]."""
    out = []
    with Image.open(path) as im:
        for k in range(n_levels + 1):
            im.seek(k)
            out.append(np.array(im))
        try:
            im.seek(n_levels + 1)
        except EOFError:
            pass
        else:
            raise AssertionError("%s has more than %d overview levels" % (path, n_levels))
    return out


def check_raster(path, T, key, block, r, strip_rows=DEFAULT_STRIP_ROWS, resampling=None, n_levels=0,
                 nearest_keys=None, band=4096):
    """Every pixel of raster r of a block (key: its pairs) in the file at path, and with resampling "average" or
    "nearest" every overview level (nearest_keys: nearest_level(key, k) for k = 1 .. n_levels)."""
    levels = decode_levels(path, n_levels if resampling else 0)
    H, W = key.shape
    full = levels[0]
    if full.shape != (H, W):
        raise AssertionError("%s is %s, want %s" % (path, full.shape, (H, W)))
    step = max(band >> n_levels, 1) << n_levels
    for y0 in range(0, H, step):
        want = expected_rows(T, key[y0:y0 + step], r)
        compare(full[y0:y0 + step], want, block, r, y0, 0, strip_rows, path)
        if resampling == "average":
            for k, lv in enumerate(average_levels(want, n_levels, band=step), 1):
                compare(levels[k][y0 >> k:(y0 >> k) + lv.shape[0]], lv, block, r, y0 >> k, k, strip_rows, path)
    for k in range(1, len(levels)):
        if levels[k].shape != (math.ceil(H / 2 ** k), math.ceil(W / 2 ** k)):
            raise AssertionError("%s level %d is %s" % (path, k, levels[k].shape))
        if resampling == "nearest":
            compare(levels[k], expected_rows(T, nearest_keys[k - 1], r), block, r, 0, k, strip_rows, path)


# ---- GDAL statistics tags --------------------------------------------------------------------------------------

ITEM = re.compile(r'<Item name="STATISTICS_([A-Z_]+)" sample="0">([^<]*)</Item>')


def check_tags(path, counts, nodata, stats=True):
    """The file's GDAL_METADATA (42112) and GDAL_NODATA (42113) tags against the statistics of a raster whose
    histogram is counts (256 bins)."""
    import pytest
    with Image.open(path) as im:
        tags = dict(im.tag_v2)
    if nodata is None:
        assert 42113 not in tags
    else:
        assert tags[42113] == str(nodata)
    counts = np.array(counts, dtype=np.int64)
    total = int(counts.sum())
    if nodata is not None:
        counts[nodata] = 0
    n = int(counts.sum())
    items = dict(ITEM.findall(tags.get(42112, "")))
    if not stats:
        assert 42112 not in tags
        return
    if n == 0:
        assert not items
        return
    vals = np.arange(256, dtype=np.float64)
    mean = float((counts * vals).sum() / n)
    std = float(np.sqrt((counts * (vals - mean) ** 2).sum() / n))
    nz = np.nonzero(counts)[0]
    assert set(items) == {"MAXIMUM", "MEAN", "MINIMUM", "STDDEV", "VALID_PERCENT"}, path
    assert float(items["MINIMUM"]) == nz[0] and float(items["MAXIMUM"]) == nz[-1], path
    assert items["VALID_PERCENT"] == "%.4g" % (100.0 * n / total), path
    assert float(items["MEAN"]) == pytest.approx(mean, rel=1e-12), path
    assert float(items["STDDEV"]) == pytest.approx(std, rel=1e-12, abs=1e-12), path
