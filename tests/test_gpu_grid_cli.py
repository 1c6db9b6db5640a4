"""GPU: the model-grid run mode end to end.  The two-block world of tests/test_gpu_aggregate_cli.py, built the same way
here -- 700 x 500 px of DEFLATE landcover at the real pixel size with a patch of landcover NoData, LZW soil 25 times
coarser, blocks 7 and 8 meeting at x = 10.028 with windows that share a pixel column -- and what
`bin/gcn10 --grid 9.9995,50.0005,0.0021,0.0021,30,22` writes under cn_grid_<cond>/: cells of 25.2 px that reach beyond
the data and the blocks on all sides, cell column 13 astride the seam.

Expected: the oracle's process_block_mem rasters of each block, masked with zoneutil.own_mask, accumulated over both
blocks with np.add.at by the numpy statement of the membership rule (tests/gridutil.py), then the mean rule."""
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

from gcn10_amd import host
from oracle import cn_oracle_c as oc
from tests import gridutil as gu
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
GRID_TEXT = "9.9995,50.0005,0.0021,0.0021,30,22"
GRID = dict(xmin=float("9.9995"), ymax=float("50.0005"), dx=float("0.0021"), dy=float("0.0021"), nx=30, ny=22)
NX, NY = 30, 22
SPLIT = 400             # the landcover as a VRT of two tiles: columns [0, 400) and [400, 700); block 7 reads the first only


def _run(cwd, *args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([GCN10, *args], cwd=str(cwd), capture_output=True, text=True, timeout=300, env=e)


def _name(r):
    c, k = divmod(r, 9)
    return os.path.join("cn_grid_%s" % CONDS[c], "cn_%s_%s.tif" % (HCS[k // 3], ARCS[k % 3]))


def _config(d, name, esa="esa.tif", extra=""):
    """a run directory of its own, with its config and log directory"""
    (d / name).mkdir()
    (d / name / "config.txt").write_text(
        "hysogs_data_path=%s\nesa_data_path=%s\nblocks_shp_path=%s\nlookup_table_path=%s\nio_threads=4\nlog_dir=%s\n%s"
        % (d / "soil.tif", d / esa, d / "blocks.shp", LOOKUPS, d / name / "logs", extra))
    return d / name


def _sums(world, bids):
    """int64[18][NY][NX][2] = {s, n} over the owned pixels of the blocks, and the owned pixels per cell and block"""
    acc = np.zeros((18, NY, NX, 2), np.int64)
    pixels = {}
    for bid in bids:
        b = world["blocks"][bid]
        kx, ky = gu.cells(GRID, b["gt"], b["W"], b["H"])
        m = zoneutil.own_mask(b["gt"], b["W"], b["H"], b["bbox"])
        assert (m == (m.any(axis=1)[:, None] & m.any(axis=0)[None, :])).all()       # a rectangle
        kx, ky = np.where(m.any(axis=0), kx, -1), np.where(m.any(axis=1), ky, -1)
        for r in range(18):
            gu.add_sums(acc[r], b["cn"][r], kx, ky)
        count = np.zeros((NY, NX, 2), np.int64)
        gu.add_sums(count, np.zeros((b["H"], b["W"]), np.uint8), kx, ky)
        pixels[bid] = count[..., 1]
    return acc, pixels


def _read(path):
    with Image.open(path) as im:
        return dict(im.tag_v2), np.array(im)


def _check_files(run_dir, want, nodata):
    for r in range(18):
        path = str(run_dir / _name(r))
        tags, got = _read(path)
        assert (tags[256], tags[257]) == (NX, NY), path
        assert (tags[322], tags[323]) == (256, 256) and tags[258] == (8,) and tags[259] == 8 and len(tags[324]) == 1, path
        assert tuple(tags[33550]) == (GRID["dx"], GRID["dy"], 0.0), path                            # ModelPixelScale
        assert tuple(tags[33922]) == (0.0, 0.0, 0.0, GRID["xmin"], GRID["ymax"], 0.0), path         # ModelTiepoint
        assert 34735 in tags, path                      # the landcover's geo keys
        assert 42112 not in tags, path
        if nodata is None:
            assert 42113 not in tags, path
        else:
            assert tags[42113] == str(nodata), path
        bad = np.argwhere(got != want[r])
        assert bad.size == 0, "%s: %d cells differ, first %s: got %d, want %d" % (
            path, len(bad), bad[0], got[tuple(bad[0])], want[r][tuple(bad[0])])
    dirs = sorted(f for f in os.listdir(run_dir) if f.startswith("cn_"))
    assert dirs == ["cn_grid_drained", "cn_grid_undrained"]             # and no cn_rasters_* directory
    for sub in dirs:
        assert len(os.listdir(run_dir / sub)) == 9 and not [f for f in os.listdir(run_dir / sub) if ".part" in f]


@pytest.fixture(scope="module")
def world(tmp_path_factory, tables):
    d = tmp_path_factory.mktemp("grid")
    rng = np.random.default_rng(11)
    small = rng.choice(ESA_NASTY, size=(RY // 20, RX // 20))
    esa = np.repeat(np.repeat(small, 20, axis=0), 20, axis=1)
    noise = rng.integers(0, 256, size=esa.shape, dtype=np.uint8)
    esa = np.where(noise < 40, rng.choice(ESA_NASTY, size=esa.shape), esa).astype(np.uint8)
    esa[300:380, 100:260] = 0               # landcover NoData: cells without a valid pixel
    soil = rng.choice(HSG_NASTY, size=(28, 36)).astype(np.uint8)
    tiffutil.write_tiff(str(d / "esa.tif"), esa, gt=ESA_GT, compression=8, tile=(256, 256))
    tiffutil.write_tiff(str(d / "soil.tif"), soil, gt=SOIL_GT, compression=5, rows_per_strip=8)
    tiffutil.write_block_shapefile(str(d / "blocks"), BLOCKS)
    # the same landcover as a VRT of two tiles, for the run that loses one of them
    (d / "tiles").mkdir()
    src = ""
    for name, x0, x1 in (("T_W.tif", 0, SPLIT), ("T_E.tif", SPLIT, RX)):
        tiffutil.write_tiff(str(d / "tiles" / name), esa[:, x0:x1], compression=8, tile=(256, 256))
        src += ('<ComplexSource resampling="nearest"><SourceFilename relativeToVRT="0">/vsicurl/https://example.invalid/'
                'map/%s</SourceFilename><SourceBand>1</SourceBand><SrcRect xOff="0" yOff="0" xSize="%d" ySize="%d" />'
                '<DstRect xOff="%d" yOff="0" xSize="%d" ySize="%d" /><NODATA>0</NODATA></ComplexSource>\n'
                % (name, x1 - x0, RY, x0, x1 - x0, RY))
    (d / "esa.vrt").write_text(
        '<VRTDataset rasterXSize="%d" rasterYSize="%d">\n<GeoTransform> %r, %r, 0.0, %r, 0.0, %r</GeoTransform>\n'
        '<VRTRasterBand dataType="Byte" band="1"><NoDataValue>0</NoDataValue>\n%s</VRTRasterBand></VRTDataset>\n'
        % (RX, RY, ESA_GT[0], ESA_GT[1], ESA_GT[3], ESA_GT[5], src))
    blocks = {}
    for bid, *bbox in BLOCKS:
        xo, yo, W, H, gt = oc.window(ESA_GT, RX, RY, bbox)
        sxo, syo, hsx, hsy, sgt = oc.window(SOIL_GT, soil.shape[1], soil.shape[0], bbox)
        cn = oc.process_block_mem(esa[yo:yo + H, xo:xo + W], gt, soil[syo:syo + hsy, sxo:sxo + hsx], sgt, tables)
        blocks[bid] = dict(xo=xo, yo=yo, W=W, H=H, gt=gt, bbox=bbox, cn=cn)
    assert blocks[7]["xo"] + blocks[7]["W"] == blocks[8]["xo"] + 1         # the windows share one pixel column
    assert blocks[7]["xo"] + blocks[7]["W"] <= SPLIT                       # block 7 lies in the first tile
    w = {"dir": d, "blocks": blocks}
    base = _config(d, "base")
    w["base"] = _run(base, "-c", "config.txt", "--grid", GRID_TEXT)
    w["both"], w["pixels"] = _sums(w, (7, 8))
    return w


def test_the_world_means_something(world):
    """Cells fed by both blocks, cells without a valid pixel outside the data and inside the NoData patch, partly valid
    cells (no GPU work)."""
    acc, pixels = world["both"], world["pixels"]
    both = (pixels[7] > 0) & (pixels[8] > 0)
    total = pixels[7] + pixels[8]
    n = acc[..., 1]
    assert both.sum() > 0 and both[:, 13].any() and not both[:, :13].any() and not both[:, 14:].any()
    assert (total == 0).sum() > 0                               # outside the data and the blocks
    assert ((total > 0)[None] & (n == 0)).all(axis=0).sum() > 0         # inside the NoData patch: pixels, none valid
    assert ((n > 0) & (n < total[None])).sum() > 0              # partly valid
    assert total.sum() == sum(int(zoneutil.own_mask(b["gt"], b["W"], b["H"], b["bbox"]).sum())
                              for b in world["blocks"].values()) - int(_outside(world))
    s = acc[..., 0]
    assert ((n > 0) & ((2 * s + n) % (2 * np.maximum(n, 1)) == 0)).sum() > 0        # exact halves


def _outside(world):
    """owned pixels that lie in no cell"""
    out = 0
    for b in world["blocks"].values():
        kx, ky = gu.cells(GRID, b["gt"], b["W"], b["H"])
        m = zoneutil.own_mask(b["gt"], b["W"], b["H"], b["bbox"])
        out += int((m & ~((ky >= 0)[:, None] & (kx >= 0)[None, :])).sum())
    return out


def test_the_rasters_of_both_blocks(world):
    out, d = world["base"], world["dir"]
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    want = gu.means(world["both"])
    _check_files(d / "base", want, None)
    log = "".join((d / "base" / "logs" / f).read_text() for f in os.listdir(d / "base" / "logs"))
    for bid, b in world["blocks"].items():
        p = host.grid_plan_block(GRID, b["W"], b["H"], b["gt"], b["bbox"])
        assert p["shared"].size > 0
        assert "grid block %d: cells [%d, %d) x [%d, %d), %d shared with other blocks" % (
            bid, p["cx0"], p["cx1"], p["cy0"], p["cy1"], p["shared"].size) in log
    empty = int((want == 255).all(axis=0).sum())
    assert empty > 0
    assert ("grid: 2 blocks, 18 rasters of 30 x 22 cells, %d cells without a valid pixel, under cn_grid_<cond>/" % empty
            in out.stdout + out.stderr)
    assert "ERROR" not in log


def test_block_order_workers_and_the_nodata_tag_do_not_change_a_pixel(world):
    d = world["dir"]
    want = gu.means(world["both"])
    first = [_read(str(d / "base" / _name(r)))[1] for r in range(18)]
    rev = _config(d, "reversed", extra="nodata=255\ncog=1\nstats=1\n")      # cog and stats play no part
    (rev / "blocks.txt").write_text("8\n7\n")
    out = _run(rev, "-c", "config.txt", "-l", "blocks.txt", "--grid", GRID_TEXT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    _check_files(rev, want, 255)
    two = _config(d, "two", extra="grid=%s\n" % GRID_TEXT)                  # the key instead of the flag
    out = _run(two, "-c", "config.txt", "--gpus", "2", env={"GCN10_OVERSUBSCRIBE": "1"})
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    _check_files(two, want, None)
    for run in (rev, two):
        for r in range(18):
            np.testing.assert_array_equal(_read(str(run / _name(r)))[1], first[r])


def test_a_list_with_block_7_alone(world):
    d = world["dir"]
    one = _config(d, "one")
    (one / "blocks.txt").write_text("7\n")
    out = _run(one, "-c", "config.txt", "-l", "blocks.txt", "--grid", GRID_TEXT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    acc, _ = _sums(world, (7,))
    want = gu.means(acc)
    _check_files(one, want, None)
    assert (want[:, :, 14:] == 255).all()                       # east of the seam nothing was processed
    # the seam column holds block 7's share only
    both = gu.means(world["both"])
    assert (want[:, :, 13] != 255).any() and (acc[:, :, 13, 1] < world["both"][:, :, 13, 1]).any()
    assert (want[:, :, :13] == both[:, :, :13]).all()
    assert "grid: 1 blocks, 18 rasters of 30 x 22 cells" in out.stdout + out.stderr


def test_an_unreadable_block_ends_with_1_after_the_rasters_are_written(world):
    """The landcover as a VRT of two tiles, the eastern one removed: block 8 cannot be read."""
    d = world["dir"]
    lost = _config(d, "lost", esa="esa.vrt", extra="esa_tile_dir=%s\n" % (d / "tiles"))
    os.remove(d / "tiles" / "T_E.tif")
    out = _run(lost, "-c", "config.txt", "--grid", GRID_TEXT)
    text = out.stdout + out.stderr
    assert out.returncode == 1, text[-2000:]
    assert "grid block 8: its landcover or soil window could not be read; the rasters lack this block" in text
    log = "".join((lost / "logs" / f).read_text() for f in os.listdir(lost / "logs"))
    assert "[ERROR]" in log and "esa load failed for block 8" in log
    acc, _ = _sums(world, (7,))
    _check_files(lost, gu.means(acc), None)
    assert "grid: 1 blocks, 18 rasters of 30 x 22 cells" in text
