"""GPU: the pair histogram of the band statistics (gcn10_gpu_pair_histogram) against numpy counts of the same
landcover and soil codes, and the program end to end with stats=1 / nodata=<v>: every written raster's GDAL tags
against the statistics numpy computes from that raster's decoded pixels."""
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

from gcn10_amd import gpu, host
from oracle import cn_oracle_c as oc
from tests import cogcheck, fullblock, tiffutil
from tests.conftest import LOOKUPS, ROOT
from tests.util import ESA_NASTY, HSG_NASTY

pytestmark = pytest.mark.gpu

GCN10 = os.path.join(ROOT, "bin", "gcn10")
CONDS, HCS, ARCS = ("drained", "undrained"), ("p", "f", "g"), ("i", "ii", "iii")
ESA_GT = [10.0, 0.001, 0.0, 50.0, 0.0, -0.001]
SOIL_GT = [9.9875, 0.025, 0.0, 50.0125, 0.0, -0.025]
BLOCKS = [(101, 10.0, 49.0, 11.0, 50.0),
          (102, 11.0, 48.0, 12.0, 49.0),
          (103, 12.5, 47.5, 13.5, 48.5),       # cut by the landcover's edge: 500 px wide
          (105, 11.3, 49.6, 11.5, 49.85),      # 200 x 250: no overview level
          (106, 10.5, 48.2, 10.7, 48.8)]
IDS = "106 105 101 102\n103\n"


def soil_code(h):
    h = np.asarray(h, np.int64)
    dual = (h >= 11) & (h <= 14)
    plain = np.where(h < 5, h, 5)
    return (np.where(dual, 4, plain) | (np.where(dual, h - 10, plain) << 4)).astype(np.uint8)


def model_histogram(esa, soil_rows):
    """[bin][landcover] counts of (landcover, soil code) pairs; soil_rows: the soil class of every pixel."""
    codes = gpu.pair_histogram_codes()
    lut = np.zeros(256, np.int64)
    for b in range(9):
        lut[codes[b]] = b
    key = lut[soil_code(soil_rows).reshape(-1)] * 256 + esa.reshape(-1).astype(np.int64)
    return np.bincount(key, minlength=16 * 256).astype(np.uint64)


def landcover(pattern, rows, W, rng):
    if pattern == "one pair":
        return np.full((rows, W), 30, np.uint8)
    if pattern == "nodata":
        return np.zeros((rows, W), np.uint8)
    if pattern == "iid":
        return rng.choice(ESA_NASTY, size=(rows, W)).astype(np.uint8)
    small = rng.choice(ESA_NASTY, size=((rows + 47) // 48, (W + 63) // 64))      # patchy
    return np.ascontiguousarray(np.repeat(np.repeat(small, 48, axis=0), 64, axis=1)[:rows, :W])


@pytest.mark.parametrize("W,rows", [(256, 300), (1000, 37), (1000, 513), (36001, 97), (17, 5)])
@pytest.mark.parametrize("pattern", ["one pair", "patchy", "iid", "nodata"])
def test_kernel_equals_numpy_counts(engine, W, rows, pattern):
    rng = np.random.default_rng(W + rows)
    esa = landcover(pattern, rows, W, rng)
    hsx, hsy = max(1, W // 25 + 2), max(1, rows // 25 + 2)
    coarse = rng.choice(HSG_NASTY, size=(hsy, hsx)).astype(np.uint8)
    if pattern == "one pair":
        coarse[:] = 3
    gt = [0.0, 1.0 / W, 0.0, 1.0, 0.0, -1.0 / W]
    sgt = [-0.013, 1.0 / (hsx - 1.5), 0.0, 1.02, 0.0, -1.0 / (hsy - 1.5)]
    ci, cj = host.build_index_maps(gt, sgt, W, rows, hsx, hsy)
    want = model_histogram(esa, coarse[cj[:, None], ci[None, :]])
    bufs = [engine.upload(a) for a in (esa, coarse, ci, cj)]
    hist = engine.alloc(16 * 256 * 8)
    try:
        engine.prepare_tile(bufs[1].ptr, hsx, hsy, bufs[2].ptr, W)
        engine.memset(hist.ptr, 0, 16 * 256 * 8)
        engine.pair_histogram(bufs[0].ptr, W, rows, bufs[3].ptr, hist.ptr)
        one = engine.download(hist.ptr, (16 * 256,), np.uint64)
        # strip by strip into the same histogram: the same counts
        engine.memset(hist.ptr, 0, 16 * 256 * 8)
        for y0 in range(0, rows, 29):
            n = min(29, rows - y0)
            engine.pair_histogram(bufs[0].ptr + y0 * W, W, n, bufs[3].ptr + 4 * y0, hist.ptr)
        strips = engine.download(hist.ptr, (16 * 256,), np.uint64)
    finally:
        for b in bufs + [hist]:
            b.close()
    np.testing.assert_array_equal(one, want)
    np.testing.assert_array_equal(strips, want)
    assert int(one.sum()) == W * rows


def test_kernel_refuses_an_unprepared_width(engine):
    esa = engine.upload(np.zeros((4, 64), np.uint8))
    cj = engine.upload(np.zeros(4, np.int32))
    hist = engine.alloc(16 * 256 * 8)
    try:
        coarse = engine.upload(np.ones((2, 2), np.uint8))
        ci = engine.upload(np.zeros(32, np.int32))
        engine.prepare_tile(coarse.ptr, 2, 2, ci.ptr, 32)
        with pytest.raises(RuntimeError, match="prepare"):
            engine.pair_histogram(esa.ptr, 64, 4, cj.ptr, hist.ptr)
        coarse.close()
        ci.close()
    finally:
        for b in (esa, cj, hist):
            b.close()


# ---- the program end to end ------------------------------------------------------------------------------------

def _world(tmp_path, seed=5, extra_cfg=""):
    rng = np.random.default_rng(seed)
    small = rng.choice(ESA_NASTY, size=(2000 // 20, 3000 // 20))
    esa = np.repeat(np.repeat(small, 20, axis=0), 20, axis=1)
    noise = rng.integers(0, 256, size=esa.shape, dtype=np.uint8)
    esa = np.where(noise < 30, rng.choice(ESA_NASTY, size=esa.shape), esa).astype(np.uint8)
    esa[:400, 300:700] = 0                  # part of block 101 is landcover NoData
    soil = rng.choice(HSG_NASTY, size=(2000 // 25 + 2, 3000 // 25 + 2)).astype(np.uint8)
    tiffutil.write_tiff(str(tmp_path / "esa.tif"), esa, gt=ESA_GT, compression=8, tile=(512, 512))
    tiffutil.write_tiff(str(tmp_path / "soil.tif"), soil, gt=SOIL_GT, compression=8, tile=(64, 64))
    tiffutil.write_block_shapefile(str(tmp_path / "blocks"), BLOCKS)
    (tmp_path / "config.txt").write_text(
        "hysogs_data_path=%s\nesa_data_path=%s\nblocks_shp_path=%s\nlookup_table_path=%s\nlog_dir=%s\n"
        "strip_rows=256\nio_threads=4\nworkers_per_gpu=1\n%s"
        % (tmp_path / "soil.tif", tmp_path / "esa.tif", tmp_path / "blocks.shp", LOOKUPS, tmp_path / "logs",
           extra_cfg))
    (tmp_path / "ids.txt").write_text(IDS)
    return esa, soil


def _run(tmp_path, *args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([GCN10, *args], cwd=str(tmp_path), capture_output=True, text=True, env=e, timeout=600)


def check_tags(path, px, nodata, stats=True):
    """The file's 42112 / 42113 against numpy's statistics of its decoded pixels px."""
    fullblock.check_tags(path, np.bincount(px.reshape(-1), minlength=256), nodata, stats)


def _check_outputs(tmp_path, esa, soil, tables, nodata, cog, sel=range(18), stats=True):
    n = 0
    for bid, *bbox in BLOCKS:
        xo, yo, W, H, gt = oc.window(ESA_GT, 3000, 2000, bbox)
        sxo, syo, hsx, hsy, sgt = oc.window(SOIL_GT, soil.shape[1], soil.shape[0], bbox)
        want = oc.process_block_mem(esa[yo:yo + H, xo:xo + W], gt, soil[syo:syo + hsy, sxo:sxo + hsx], sgt, tables)
        for r in sel:
            c, k = divmod(r, 9)
            p = str(tmp_path / ("cn_rasters_%s" % CONDS[c]) / ("cn_%s_%s_%d.tif" % (HCS[k // 3], ARCS[k % 3], bid)))
            with Image.open(p) as im:
                px = np.array(im)
            np.testing.assert_array_equal(px, want[r], err_msg=p)
            check_tags(p, px, nodata, stats)
            if cog:
                ifds = cogcheck.check_cog(p)
                for j, (_p, _e, t, _r) in enumerate(ifds):
                    assert (42112 in t) == (j == 0 and stats)
                    assert (42113 in t) == (nodata is not None)
            n += 1
    return n


MODES = [("gpu_deflate=2\n", False), ("gpu_deflate=1\n", False), ("gpu_deflate=0\n", False),
         ("compress=lzw\n", False), ("cog=1\n", True), ("cog=1\noverview_resampling=average\ncompress=lzw\n", True)]


@pytest.mark.parametrize("mode,cog", MODES)
@pytest.mark.parametrize("nodata", [None, 255])
def test_run_writes_the_statistics_of_every_raster(tmp_path, tables, mode, cog, nodata):
    extra = mode + "stats=1\n" + ("nodata=%d\n" % nodata if nodata is not None else "")
    esa, soil = _world(tmp_path, extra_cfg=extra)
    out = _run(tmp_path, "-c", "config.txt", "-l", "ids.txt")
    assert out.returncode == 0, out.stderr[-2000:]
    log = (tmp_path / "logs" / "rank_0.log").read_text()
    assert "processed 5 blocks" in log
    assert (", stats, nodata 255" if nodata is not None else ", stats;") in log
    assert _check_outputs(tmp_path, esa, soil, tables, nodata, cog) == 90


def test_flags_subset_and_nodata_without_statistics(tmp_path, tables):
    esa, soil = _world(tmp_path, seed=9, extra_cfg="nodata=255\n")
    # --nodata overrides the config key; --stats turns them on; a lookup subset gets tags on its rasters only
    out = _run(tmp_path, "-c", "config.txt", "-l", "ids.txt", "--stats", "--nodata", "0", "--lookups", "g_ii,p_i",
               "--conditions", "undrained")
    assert out.returncode == 0, out.stderr[-2000:]
    assert not (tmp_path / "cn_rasters_drained").exists()
    assert _check_outputs(tmp_path, esa, soil, tables, 0, False, sel=[9, 16]) == 10
    assert len(os.listdir(tmp_path / "cn_rasters_undrained")) == 10
    # nodata alone: the NoData tag, no statistics
    for d in ("cn_rasters_undrained",):
        for f in os.listdir(tmp_path / d):
            os.remove(tmp_path / d / f)
    out = _run(tmp_path, "-c", "config.txt", "-l", "ids.txt", "-o", "--lookups", "g_ii", "--conditions", "undrained")
    assert out.returncode == 0, out.stderr[-2000:]
    assert _check_outputs(tmp_path, esa, soil, tables, 255, False, sel=[16], stats=False) == 5


def test_full_size_block_of_the_real_vrt_shape(tmp_path, tables):
    """36001 x 36001 with stats=1 and nodata=255: three rasters' tags against numpy on their decoded pixels."""
    import bench
    Image.MAX_IMAGE_PIXELS = None
    size, px = 36001, 8.3333333333330430e-05
    esa, _, coarse, _ = bench.synth_block(5, size, "patches")
    hs = coarse.shape[0]
    egt = [0.0, px, 0.0, 3.0, 0.0, -px]
    sgt = [0.0, 3.0 / hs, 0.0, 3.0, 0.0, -3.0 / hs]
    tiffutil.write_tiff(str(tmp_path / "esa.tif"), esa, gt=egt, compression=8, tile=(1024, 1024))
    del esa
    tiffutil.write_tiff(str(tmp_path / "soil.tif"), coarse, gt=sgt, compression=5, rows_per_strip=16)
    tiffutil.write_block_shapefile(str(tmp_path / "blocks"), [(1, 0.0, 0.0, 3.0, 3.0)])
    (tmp_path / "config.txt").write_text(
        "hysogs_data_path=%s\nesa_data_path=%s\nblocks_shp_path=%s\nlookup_table_path=%s\nlog_dir=%s\nstats=1\n"
        "nodata=255\n" % (tmp_path / "soil.tif", tmp_path / "esa.tif", tmp_path / "blocks.shp", LOOKUPS,
                          tmp_path / "logs"))
    out = _run(tmp_path, "-c", "config.txt")
    assert out.returncode == 0, out.stderr[-2000:]
    for r in (0, 13, 17):
        c, k = divmod(r, 9)
        p = str(tmp_path / ("cn_rasters_%s" % CONDS[c]) / ("cn_%s_%s_1.tif" % (HCS[k // 3], ARCS[k % 3])))
        with Image.open(p) as im:
            a = np.array(im)
        assert a.shape == (size, size)
        check_tags(p, a, 255)
        del a
