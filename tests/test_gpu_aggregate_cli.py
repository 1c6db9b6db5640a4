"""GPU: the aggregate run mode end to end.  The small world of tests/test_gpu_zonal_cli.py -- DEFLATE landcover in
256^2 tiles at the real pixel size, LZW soil 25 times coarser, two adjacent blocks whose windows share a pixel
column -- and what `bin/gcn10 --aggregate 25` and `aggregate=7` with compress=lzw write under cn_rasters_<cond>_x<f>/
against the oracle's 18 rasters of each block, reduced in numpy over the block's owned pixels (tests/aggutil.py)."""
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

from gcn10_amd import host
from oracle import cn_oracle_c as oc
from tests import aggutil as au
from tests import tiffutil, zoneutil
from tests.conftest import LOOKUPS, ROOT
from tests.util import ESA_NASTY, HSG_NASTY

pytestmark = pytest.mark.gpu

GCN10 = os.path.join(ROOT, "bin", "gcn10")
CONDS, HCS, ARCS = ("drained", "undrained"), ("p", "f", "g"), ("i", "ii", "iii")
PX = 8.3333333333330430e-05
RX, RY = 700, 500
ESA_GT = [10.0, PX, 0.0, 50.0, 0.0, -PX]
SOIL_GT = [9.99, 25 * PX, 0.0, 50.01, 0.0, -25 * PX]
BLOCKS = [(7, 10.0, 49.96, 10.028, 50.0), (8, 10.028, 49.96, 10.056, 50.0)]


def _run(cwd, *args):
    return subprocess.run([GCN10, *args], cwd=str(cwd), capture_output=True, text=True, timeout=300)


def _name(r, bid, f, tail=""):
    c, k = divmod(r, 9)
    return os.path.join("cn_rasters_%s_x%d" % (CONDS[c], f), "cn_%s_%s_%d%s.tif" % (HCS[k // 3], ARCS[k % 3], bid, tail))


@pytest.fixture(scope="module")
def world(tmp_path_factory, tables):
    d = tmp_path_factory.mktemp("aggregate")
    rng = np.random.default_rng(11)
    small = rng.choice(ESA_NASTY, size=(RY // 20, RX // 20))
    esa = np.repeat(np.repeat(small, 20, axis=0), 20, axis=1)
    noise = rng.integers(0, 256, size=esa.shape, dtype=np.uint8)
    esa = np.where(noise < 40, rng.choice(ESA_NASTY, size=esa.shape), esa).astype(np.uint8)
    esa[300:380, 100:260] = 0               # landcover NoData: cells without a valid pixel at either factor
    soil = rng.choice(HSG_NASTY, size=(28, 36)).astype(np.uint8)
    tiffutil.write_tiff(str(d / "esa.tif"), esa, gt=ESA_GT, compression=8, tile=(256, 256))
    tiffutil.write_tiff(str(d / "soil.tif"), soil, gt=SOIL_GT, compression=5, rows_per_strip=8)
    tiffutil.write_block_shapefile(str(d / "blocks"), BLOCKS)
    base = ("hysogs_data_path=%s\nesa_data_path=%s\nblocks_shp_path=%s\nlookup_table_path=%s\nio_threads=4\n"
            % (d / "soil.tif", d / "esa.tif", d / "blocks.shp", LOOKUPS))
    (d / "config1.txt").write_text(base + "log_dir=%s\n" % (d / "logs1"))
    (d / "config2.txt").write_text(base + "log_dir=%s\naggregate=7\ncompress=lzw\nnodata=255\nstats=1\ncog=1\n"
                                   "gpu_deflate=1\n" % (d / "logs2"))
    blocks = {}
    for bid, *bbox in BLOCKS:
        xo, yo, W, H, gt = oc.window(ESA_GT, RX, RY, bbox)
        sxo, syo, hsx, hsy, sgt = oc.window(SOIL_GT, soil.shape[1], soil.shape[0], bbox)
        cn = oc.process_block_mem(esa[yo:yo + H, xo:xo + W], gt, soil[syo:syo + hsy, sxo:sxo + hsx], sgt, tables)
        m = zoneutil.own_mask(gt, W, H, bbox)               # the owned rectangle by the rule itself, in numpy
        xs, ys = np.flatnonzero(m.any(axis=0)), np.flatnonzero(m.any(axis=1))
        blocks[bid] = dict(xo=xo, yo=yo, W=W, H=H, gt=gt, bbox=bbox, cn=cn, x0=int(xs[0]), x1=int(xs[-1]) + 1,
                           y0=int(ys[0]), y1=int(ys[-1]) + 1)
    assert blocks[7]["xo"] + blocks[7]["W"] == blocks[8]["xo"] + 1         # the windows share one pixel column
    assert blocks[7]["xo"] + blocks[7]["x1"] == blocks[8]["xo"] + blocks[8]["x0"]   # ... which only one of them owns
    return {"dir": d, "blocks": blocks, "run25": _run(d, "-c", "config1.txt", "--aggregate", "25")}


def _check_file(path, b, r, f, compression, nodata):
    g = host.aggregate_geometry(b["W"], b["H"], b["gt"], b["bbox"], f)
    assert (g["x0"], g["x1"], g["y0"], g["y1"]) == (b["x0"], b["x1"], b["y0"], b["y1"])
    want = au.reduce_raster(b["cn"][r][b["y0"]:b["y1"]], b["x0"], b["x1"], f)
    assert want.shape == (g["Ha"], g["Wa"])
    with Image.open(path) as im:
        tags = dict(im.tag_v2)
        got = np.array(im)
    assert (tags[256], tags[257]) == (g["Wa"], g["Ha"]), path
    assert (tags[322], tags[323]) == (256, 256) and tags[258] == (8,) and tags[259] == compression, path
    assert len(tags[324]) == -(-g["Wa"] // 256) * -(-g["Ha"] // 256)
    assert tuple(tags[33550]) == (g["gt"][1], -g["gt"][5], 0.0), path                # ModelPixelScale
    assert tuple(tags[33922]) == (0.0, 0.0, 0.0, g["gt"][0], g["gt"][3], 0.0), path  # ModelTiepoint
    assert g["gt"][1] == f * PX and g["gt"][0] == b["gt"][0] + b["x0"] * PX
    if nodata is None:
        assert 42113 not in tags, path
    else:
        assert tags[42113] == str(nodata), path
    assert 42112 not in tags, path                  # no statistics on aggregated rasters
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d cells differ, first %s" % (path, len(bad), bad[0])
    return want


def test_aggregate_25_writes_the_reduced_oracle_rasters(world):
    out, d = world["run25"], world["dir"]
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    empty = partial = 0
    for bid, b in world["blocks"].items():
        for r in range(18):
            _check_file(str(d / _name(r, bid, 25)), b, r, 25, 8, None)
            s, n, area = au.reduce_sums(b["cn"][r][b["y0"]:b["y1"]], b["x0"], b["x1"], 25)
            empty += int((n == 0).sum())
            partial += int(((n > 0) & (n < area)).sum())
    assert empty > 0 and partial > 0                # the world means something
    dirs = sorted(f for f in os.listdir(d) if f.startswith("cn_rasters"))
    assert dirs == ["cn_rasters_drained_x25", "cn_rasters_undrained_x25"]
    for sub in dirs:
        assert len(os.listdir(d / sub)) == 18 and not [f for f in os.listdir(d / sub) if ".part" in f]
    log = "".join((d / "logs1" / f).read_text() for f in os.listdir(d / "logs1"))
    for bid, b in world["blocks"].items():
        g = host.aggregate_geometry(b["W"], b["H"], b["gt"], b["bbox"], 25)
        assert "aggregate block %d: %d x %d cells of 25 x 25 px" % (bid, g["Wa"], g["Ha"]) in log
    assert "aggregate: 2 blocks, 18 rasters each, cells of 25 x 25 px" in out.stdout + out.stderr


def test_the_two_blocks_abut_without_sharing_a_cell(world):
    b7, b8 = world["blocks"][7], world["blocks"][8]
    g7 = host.aggregate_geometry(b7["W"], b7["H"], b7["gt"], b7["bbox"], 25)
    g8 = host.aggregate_geometry(b8["W"], b8["H"], b8["gt"], b8["bbox"], 25)
    # in mosaic pixels: block 7's last owned column is the one before block 8's first, and the rows are the same
    assert b7["xo"] + g7["x1"] == b8["xo"] + g8["x0"]
    assert (b7["yo"] + g7["y0"], b7["yo"] + g7["y1"]) == (b8["yo"] + g8["y0"], b8["yo"] + g8["y1"])
    assert g7["Ha"] == g8["Ha"] and g7["gt"][3] == g8["gt"][3]
    # block 8's origin is the outer corner of its first owned pixel
    assert g8["gt"][0] == b8["gt"][0] + g8["x0"] * PX


def test_aggregate_7_from_the_config_with_lzw_and_nodata(world):
    """The key instead of the flag; LZW tiles and the GDAL_NODATA tag; cog, stats and gpu_deflate play no part."""
    d = world["dir"]
    out = _run(d, "-c", "config2.txt")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    ties = 0
    for bid, b in world["blocks"].items():
        for r in range(18):
            _check_file(str(d / _name(r, bid, 7)), b, r, 7, 5, 255)
            with Image.open(str(d / _name(r, bid, 7))) as im:
                assert getattr(im, "n_frames", 1) == 1          # no overview directories
            s, n, _ = au.reduce_sums(b["cn"][r][b["y0"]:b["y1"]], b["x0"], b["x1"], 7)
            ties += int(((n > 0) & ((2 * s + n) % (2 * np.maximum(n, 1)) == 0)).sum())
    assert ties > 0
    assert not (d / "cn_rasters_drained").exists() and not (d / "cn_rasters_undrained").exists()


def test_lookups_conditions_and_the_second_run(world):
    d = world["dir"]
    args = ("-c", "config1.txt", "--aggregate", "100", "--lookups", "g_ii", "--conditions", "drained")
    out = _run(d, *args)
    assert out.returncode == 0, out.stderr[-2000:]
    assert sorted(os.listdir(d / "cn_rasters_drained_x100")) == ["cn_g_ii_7.tif", "cn_g_ii_8.tif"]
    assert not (d / "cn_rasters_undrained_x100").exists()
    for bid, b in world["blocks"].items():
        _check_file(str(d / _name(7, bid, 100)), b, 7, 100, 8, None)
    # without -o an existing raster is left alone and the new one gets the reference's trailing underscore
    before = (d / "cn_rasters_drained_x100" / "cn_g_ii_7.tif").read_bytes()
    out = _run(d, *args)
    assert out.returncode == 0, out.stderr[-2000:]
    assert sorted(os.listdir(d / "cn_rasters_drained_x100")) == ["cn_g_ii_7.tif", "cn_g_ii_7_.tif", "cn_g_ii_8.tif",
                                                                 "cn_g_ii_8_.tif"]
    assert (d / "cn_rasters_drained_x100" / "cn_g_ii_7.tif").read_bytes() == before
    for bid, b in world["blocks"].items():
        _check_file(str(d / _name(7, bid, 100, "_")), b, 7, 100, 8, None)
    # with -o the plain names are written again
    out = _run(d, *args, "-o")
    assert out.returncode == 0 and len(os.listdir(d / "cn_rasters_drained_x100")) == 4
    assert not (d / "cn_rasters_drained").exists() and not (d / "cn_rasters_undrained").exists()
