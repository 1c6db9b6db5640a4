"""GPU: the runoff_rain run end to end (bin/gcn10 --runoff-rain ...), on the two-block world of
tests/test_gpu_zonal_cli.py with the raster of tests/test_gpu_zone_rain_cli.py: cells of 37.3 pixels that cover the world
partly.  Every pixel of every written file against numpy: the oracle's rasters of the block, the cell rule of the
raster's grid on the block's own pixel centres (test_gpu_zone_rain_cli._cells), and the tables of tests/runoffutil.py
through the Python model of gcn10_runoff_bytes.  The files are decoded with PIL, as the other CLI tests decode theirs."""
import os

import numpy as np
import pytest
from PIL import Image

from tests import runoffutil as ru
from tests import tiffutil
from tests.test_gpu_zonal_cli import ARCS, CONDS, HCS, _run, world  # noqa: F401  (the world)
from tests.test_gpu_zone_rain_cli import ATLAS, _cells, _config, _gt
from tests.test_runoff_raster_host import model_bytes

pytestmark = pytest.mark.gpu

UNIT, LAM = 2.5, 0.2
GEO_TAGS = (256, 257, 258, 259, 322, 323, 33550, 33922)     # size, bits, compression, tile size, pixel scale, tiepoint


def _name(r, bid, tail=""):
    c, k = divmod(r, 9)
    return os.path.join("runoff_rasters_%s" % CONDS[c], "q_%s_%s_%d%s.tif" % (HCS[k // 3], ARCS[k % 3], bid, tail))


def _cn_name(r, bid):
    c, k = divmod(r, 9)
    return os.path.join("cn_rasters_%s" % CONDS[c], "cn_%s_%s_%d.tif" % (HCS[k // 3], ARCS[k % 3], bid))


def _read(path):
    with Image.open(path) as im:
        return dict(im.tag_v2), np.array(im)


def _tables(unit, lam, u):
    q = [[int(x) for x in ru.table(b * unit, lam)] for b in range(256)]
    return model_bytes(q, u)


def _want(block, g, field, t):
    """the 18 rasters of a block under the raster: t[byte of the pixel's cell][cn], 255 outside every cell"""
    _xo, _yo, W, H, gt, _bbox, cn = block
    cx, cy = _cells(g, gt, W, H)
    inside = (cy >= 0)[:, None] & (cx >= 0)[None, :]
    byte = field[np.maximum(cy, 0)[:, None], np.maximum(cx, 0)[None, :]].astype(np.int64)
    return [np.where(inside, t[byte, cn[r]], 255).astype(np.uint8) for r in range(18)], inside


@pytest.fixture(scope="module")
def runs(world):  # noqa: F811
    """the plain run, and the run under the raster"""
    d = world["dir"]
    field = np.random.default_rng(21).integers(0, 256, (ATLAS["ny"], ATLAS["nx"])).astype(np.uint8)
    field[0, :3] = (0, 255, 0)
    tiffutil.write_tiff(str(d / "runoff_atlas.tif"), field, gt=_gt(ATLAS), compression=8, tile=(16, 16))
    plain = _run(d, "-c", _config(d, 31))
    rain = _run(d, "-c", _config(d, 32), "--runoff-rain", "runoff_atlas.tif", "--runoff-rain-unit", "2.5")
    return {"field": field, "plain": plain, "rain": rain, "t": _tables(UNIT, LAM, 250)}


def _check_all(d, world, field, t, sel=range(18), tail="", compression=8):  # noqa: F811
    values = set()
    for bi, bid in enumerate((7, 8)):
        want, inside = _want(world["blocks"][bi], ATLAS, field, t)
        assert inside.any() and not inside.all(), "block %d does not lie partly under the raster" % bid
        for r in sel:
            tags, got = _read(str(d / _name(r, bid, tail)))
            assert tags[259] == compression
            bad = np.argwhere(got != want[r])
            assert bad.size == 0, "%s: %d pixels differ, first at %s" % (_name(r, bid, tail), len(bad), bad[0])
            values |= set(np.unique(got).tolist())
    return values


def test_every_pixel_of_the_18_files_equals_the_numpy_model(world, runs):  # noqa: F811
    d, out = world["dir"], runs["rain"]
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    values = _check_all(d, world, runs["field"], runs["t"])
    assert len(values) >= 20 and 255 in values, sorted(values)
    for c in CONDS:
        names = sorted(os.listdir(d / ("runoff_rasters_%s" % c)))
        assert len(names) == 18 and not [f for f in names if ".part" in f], names
    log = "".join((d / "logs32" / f).read_text() for f in os.listdir(d / "logs32"))
    line = [ln for ln in log.split("\n") if "runoff_rain: " in ln and "1 count" in ln]
    assert len(line) == 1, log[-3000:]
    assert ("runoff_atlas.tif, %d x %d cells of %.17g x %.17g from (%.17g, %.17g), unit = 2.5 mm, lambda = %.17g, "
            "1 count = 250/100 mm" % (ATLAS["nx"], ATLAS["ny"], ATLAS["dx"], ATLAS["dy"], ATLAS["xmin"], ATLAS["ymax"],
                                      LAM)) in line[0], line[0]


def test_size_geotransform_and_tile_tags_equal_the_cn_rasters(world, runs):  # noqa: F811
    d = world["dir"]
    assert runs["plain"].returncode == 0 and runs["rain"].returncode == 0
    for bid in (7, 8):
        for r in range(18):
            cn_tags, _ = _read(str(d / _cn_name(r, bid)))
            q_tags, _ = _read(str(d / _name(r, bid)))
            for tag in GEO_TAGS:
                assert q_tags[tag] == cn_tags[tag], (bid, r, tag)
            assert len(q_tags[324]) == len(cn_tags[324]) and sorted(q_tags) == sorted(cn_tags), (bid, r)


def test_lzw_decodes_to_the_same_pixels(world, runs):  # noqa: F811
    d = world["dir"]
    out = _run(d, "-c", _config(d, 33), "--runoff-rain", "runoff_atlas.tif", "--runoff-rain-unit", "2.5", "--compress",
               "lzw")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    _check_all(d, world, runs["field"], runs["t"], tail="_", compression=5)     # (the plain names exist: trailing underscore)


def test_one_lookup_and_one_condition_write_one_file(world, runs, tmp_path):  # noqa: F811
    d = world["dir"]
    sub = d / "one"
    sub.mkdir(exist_ok=True)
    out = _run(sub, "-c", str(d / _config(d, 34)), "--runoff-rain", str(d / "runoff_atlas.tif"), "--runoff-rain-unit",
               "2.5", "--runoff-unit", "1", "--lookups", "g_ii", "--conditions", "drained")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert sorted(os.listdir(sub)) == ["runoff_rasters_drained"]
    assert sorted(os.listdir(sub / "runoff_rasters_drained")) == ["q_g_ii_7.tif", "q_g_ii_8.tif"]
    t = _tables(UNIT, LAM, 100)                     # --runoff-unit 1: counts of 1 mm
    assert (t != runs["t"]).any()
    _check_all(sub, world, runs["field"], t, sel=[7])


def test_a_constant_raster_is_one_table_over_the_plain_cn_files(world, runs):  # noqa: F811
    d = world["dir"]
    b = 37
    sub = d / "const"
    sub.mkdir(exist_ok=True)
    tiffutil.write_tiff(str(d / "const.tif"), np.full((ATLAS["ny"], ATLAS["nx"]), b, np.uint8), gt=_gt(ATLAS),
                        compression=8, tile=(16, 16))
    out = _run(sub, "-c", str(d / _config(d, 35)), "--runoff-rain", str(d / "const.tif"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    t = _tables(1.0, 0.2, 100)                      # the defaults: 1 mm per count in, 1 mm per count out
    for bi, bid in enumerate((7, 8)):
        _xo, _yo, W, H, gt, _bbox, _cn = world["blocks"][bi]
        cx, cy = _cells(ATLAS, gt, W, H)
        inside = (cy >= 0)[:, None] & (cx >= 0)[None, :]
        for r in range(18):
            _, cn = _read(str(d / _cn_name(r, bid)))
            _, got = _read(str(sub / _name(r, bid)))
            np.testing.assert_array_equal(got[inside], t[b][cn[inside]])
            assert (got[~inside] == 255).all()
