"""GPU: the overview kernels (gcn10_gpu_overview_*) against a numpy model of the two resamplings, and the gcn10
program with cog=1 end to end: every output passes the COG checker, full resolution equals the oracle, every level
equals the model."""
import math
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

from gcn10_amd import host
from oracle import cn_oracle_c as oc
from tests import cogcheck, tiffutil
from tests.fullblock import average_levels, nearest_level
from tests.conftest import LOOKUPS, ROOT
from tests.util import ESA_NASTY, HSG_NASTY, make_block, random_tables

pytestmark = pytest.mark.gpu

GCN10 = os.path.join(ROOT, "bin", "gcn10")
CONDS, HCS, ARCS = ("drained", "undrained"), ("p", "f", "g"), ("i", "ii", "iii")
ESA_GT = [10.0, 0.001, 0.0, 50.0, 0.0, -0.001]
SOIL_GT = [9.9875, 0.025, 0.0, 50.0125, 0.0, -0.025]
BLOCKS = [(101, 10.0, 49.0, 11.0, 50.0),
          (102, 11.0, 48.0, 12.0, 49.0),
          (103, 12.5, 47.5, 13.5, 48.5),
          (105, 11.3, 49.6, 11.5, 49.85),      # 200 x 250: no overview level, still a COG
          (106, 10.5, 48.2, 10.7, 48.8)]       # 200 x 600: 2 levels, as wide as 105
# 106 first: the first block logs its level count; then 105, whose soil tile must be its own, not 106's
IDS = "106 105 101 102\n103\n"
GUARD = 256


# ---- the model of the two resamplings (tests/fullblock.py) ----------------------------------------------------

def test_model_rules():
    a = np.array([[10, 11, 255], [20, 255, 255]], np.uint8)
    l1 = average_levels(a, 1)[0]
    assert l1.tolist() == [[14, 255]]           # (2*41 + 3) // 6 = 14; all-255 footprint stays 255
    assert average_levels(np.array([[1, 2]], np.uint8), 1)[0].tolist() == [[2]]     # 1.5 rounds half up
    b = np.arange(25, dtype=np.uint8).reshape(5, 5)
    assert nearest_level(b, 1).tolist() == [[6, 8, 9], [16, 18, 19], [21, 23, 24]]


# ---- kernels through the C ABI --------------------------------------------------------------------------------

def _sel(cond_mask, table_mask):
    return [r for r in range(18) if (cond_mask >> (r // 9)) & 1 and (table_mask >> (r % 9)) & 1]


@pytest.mark.parametrize("H,W,nasty,tabs,cond_mask,table_mask", [
    (700, 1037, True, "random", 3, 0x1FF),
    (513, 300, True, "shipped", 1, 0x1FF),
    (1100, 600, False, "random", 2, 0b100100001),
    (257, 3, True, "random", 3, 0b10),
    (70, 2100, True, "shipped", 3, 0x1FF),
    (36001, 40, True, "random", 1, 0b1010),         # 8 levels: the reduction down to 1 x 1 per workgroup tile
    (40, 36001, True, "shipped", 3, 0b100000001),   # 8 levels across, level 8 clipped at the right edge
])
def test_average_kernel_equals_the_model(engine, tables, H, W, nasty, tabs, cond_mask, table_mask):
    t = random_tables(H + W) if tabs == "random" else tables
    esa, gt, coarse, sgt = make_block(H * 7 + W, H, W, 37, 53, nasty=nasty)
    full = oc.process_block_mem(esa, gt, coarse, sgt, t, cond_mask=cond_mask, table_mask=table_mask)
    L = host.cog_levels(W, H)
    L = max(L, 1)
    sel = _sel(cond_mask, table_mask)
    ci, cj = host.build_index_maps(gt, sgt, W, H, coarse.shape[1], coarse.shape[0])
    engine.set_tables(t)
    bufs = [engine.upload(a) for a in (esa, coarse, ci, cj)]
    sizes = [(math.ceil(H / 2 ** k), math.ceil(W / 2 ** k)) for k in range(1, L + 1)]
    offs, total = [], GUARD
    for _q in sel:
        for h, w in sizes:
            offs.append(total)
            total += h * w + GUARD
    out = engine.alloc(total)
    try:
        engine.memset(out.ptr, 0xA5, total)
        engine.prepare_tile(bufs[1].ptr, coarse.shape[1], coarse.shape[0], bufs[2].ptr, W)
        ptrs = [out.ptr + o for o in offs]
        for y0 in range(0, H, 512):         # strips of 512 rows, the last one shorter
            engine.overview_average(bufs[0].ptr, W, H, y0, min(512, H - y0), bufs[3].ptr, cond_mask, table_mask,
                                    L, ptrs)
        got = engine.download(out.ptr, (total,))
    finally:
        for b in bufs + [out]:
            b.close()
    guard = np.ones(total, bool)
    for q, r in enumerate(sel):
        model = average_levels(full[r], L)
        for k in range(L):
            h, w = sizes[k]
            o = offs[q * L + k]
            guard[o:o + h * w] = False
            np.testing.assert_array_equal(got[o:o + h * w].reshape(h, w), model[k],
                                          err_msg="raster %d level %d" % (r, k + 1))
    assert (got[guard] == 0xA5).all(), "a byte outside the level rasters was written"


@pytest.mark.parametrize("H,W", [(700, 1037), (257, 3), (1, 5000), (36001, 40)])
def test_nearest_kernel_equals_the_model(engine, H, W):
    rng = np.random.default_rng(H + W)
    esa = rng.choice(ESA_NASTY, size=(H, W)).astype(np.uint8)
    src = engine.upload(esa)
    try:
        for k in range(1, max(host.cog_levels(W, H), 1) + 1):
            h, w = math.ceil(H / 2 ** k), math.ceil(W / 2 ** k)
            out = engine.alloc(h * w + 2 * GUARD)
            try:
                engine.memset(out.ptr, 0x5A, h * w + 2 * GUARD)
                engine.overview_nearest(src.ptr, W, H, k, out.ptr + GUARD)
                got = engine.download(out.ptr, (h * w + 2 * GUARD,))
            finally:
                out.close()
            np.testing.assert_array_equal(got[GUARD:GUARD + h * w].reshape(h, w), nearest_level(esa, k))
            assert (got[:GUARD] == 0x5A).all() and (got[GUARD + h * w:] == 0x5A).all()
    finally:
        src.close()


def test_average_kernel_refuses_bad_strips(engine, tables):
    esa, gt, coarse, sgt = make_block(1, 600, 600, 20, 20)
    ci, cj = host.build_index_maps(gt, sgt, 600, 600, 20, 20)
    engine.set_tables(tables)
    bufs = [engine.upload(a) for a in (esa, coarse, ci, cj)]
    out = engine.alloc(300 * 300 * 2 + 64)
    try:
        engine.prepare_tile(bufs[1].ptr, 20, 20, bufs[2].ptr, 600)
        for y0, rows, L in ((100, 256, 2), (0, 300, 2), (0, 600, 9), (0, 600, 0)):
            with pytest.raises(Exception):
                engine.overview_average(bufs[0].ptr, 600, 600, y0, rows, bufs[3].ptr, 1, 1, L,
                                        [out.ptr] * max(L, 1))
    finally:
        for b in bufs + [out]:
            b.close()


# ---- the program end to end ------------------------------------------------------------------------------------

def _world(tmp_path, seed=5, extra_cfg=""):
    rng = np.random.default_rng(seed)
    small = rng.choice(ESA_NASTY, size=(2000 // 20, 3000 // 20))
    esa = np.repeat(np.repeat(small, 20, axis=0), 20, axis=1)
    noise = rng.integers(0, 256, size=esa.shape, dtype=np.uint8)
    esa = np.where(noise < 30, rng.choice(ESA_NASTY, size=esa.shape), esa).astype(np.uint8)
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


def _levels(path):
    out = []
    with Image.open(path) as im:
        k = 0
        while True:
            try:
                im.seek(k)
            except EOFError:
                return out
            out.append(np.array(im))
            k += 1


def _check_outputs(tmp_path, esa, soil, tables, method, compression, cond_mask=3, table_mask=0x1FF):
    n = 0
    for bid, *bbox in BLOCKS:
        xo, yo, W, H, gt = oc.window(ESA_GT, 3000, 2000, bbox)
        sxo, syo, hsx, hsy, sgt = oc.window(SOIL_GT, soil.shape[1], soil.shape[0], bbox)
        want = oc.process_block_mem(esa[yo:yo + H, xo:xo + W], gt, soil[syo:syo + hsy, sxo:sxo + hsx], sgt,
                                    tables, cond_mask=cond_mask, table_mask=table_mask)
        L = host.cog_levels(W, H)         # 2 levels; 1 for block 103 (the landcover's edge cuts it to 500 px); 0 for 105
        assert L == {101: 2, 102: 2, 103: 1, 105: 0, 106: 2}[bid]
        for r in _sel(cond_mask, table_mask):
            c, k = divmod(r, 9)
            p = str(tmp_path / ("cn_rasters_%s" % CONDS[c]) / ("cn_%s_%s_%d.tif" % (HCS[k // 3], ARCS[k % 3], bid)))
            ifds = cogcheck.check_cog(p, n_levels=L, compression=compression)
            assert tuple(ifds[0][2][33550]) == (gt[1], -gt[5], 0.0)
            got = _levels(p)
            np.testing.assert_array_equal(got[0], want[r], err_msg=p)
            model = ([nearest_level(want[r], j) for j in range(1, L + 1)] if method == "nearest"
                     else average_levels(want[r], L))
            for j in range(L):
                np.testing.assert_array_equal(got[j + 1], model[j], err_msg="%s level %d" % (p, j + 1))
            n += 1
    return n


@pytest.mark.parametrize("method", ["nearest", "average"])
@pytest.mark.parametrize("gpu_deflate", [1, 2])
@pytest.mark.parametrize("compress", ["deflate", "lzw"])
def test_cog_run_equals_oracle_and_model(tmp_path, tables, method, gpu_deflate, compress):
    esa, soil = _world(tmp_path, extra_cfg="gpu_deflate=%d\ncompress=%s\ncog=1\noverview_resampling=%s\n"
                       % (gpu_deflate, compress, method))
    out = _run(tmp_path, "-c", "config.txt", "-l", "ids.txt")
    assert out.returncode == 0, out.stderr[-2000:]
    log = (tmp_path / "logs" / "rank_0.log").read_text()
    assert "cog: Cloud Optimized GeoTIFFs, overviews by %s resampling, 2 levels" % method in log
    assert "processed 5 blocks" in log
    assert _check_outputs(tmp_path, esa, soil, tables, method, 5 if compress == "lzw" else 8) == 90


@pytest.mark.parametrize("method", ["nearest", "average"])
def test_cog_flags_direct_io_spill_and_subset(tmp_path, tables, method):
    esa, soil = _world(tmp_path, seed=9, extra_cfg="direct_io=1\n")
    out = _run(tmp_path, "-c", "config.txt", "-l", "ids.txt", "--cog", "--overview-resampling", method,
               "--lookups", "g_ii,p_i", "--conditions", "undrained", env={"GCN10_PINNED_ARENA_BYTES": "4096"})
    assert out.returncode == 0, out.stderr[-2000:]
    assert not (tmp_path / "cn_rasters_drained").exists()
    assert _check_outputs(tmp_path, esa, soil, tables, method, 8, cond_mask=2, table_mask=(1 << 7) | 1) == 10


def test_cog_null_sink_runs_the_overviews_and_writes_nothing(tmp_path):
    _world(tmp_path, extra_cfg="cog=1\noverview_resampling=average\n")
    out = _run(tmp_path, "-c", "config.txt", "-l", "ids.txt", env={"GCN10_SINK": "null"})
    assert out.returncode == 0, out.stderr[-2000:]
    log = (tmp_path / "logs" / "rank_0.log").read_text()
    assert "overviews by average resampling, 2 levels" in log and "processed 5 blocks" in log
    assert not (tmp_path / "cn_rasters_drained").exists() or not os.listdir(tmp_path / "cn_rasters_drained")


def test_cog_full_size_block_of_the_real_vrt_shape(tmp_path, tables):
    """36001 x 36001, 8 levels, nearest: the checker on three rasters, full resolution on 600 sampled rows, and
    level 8 (141 x 141) against the oracle at its sample points."""
    import bench
    Image.MAX_IMAGE_PIXELS = None
    size, px = 36001, 8.3333333333330430e-05
    esa, _, coarse, _ = bench.synth_block(5, size, "patches")
    hs = coarse.shape[0]
    egt = [0.0, px, 0.0, 3.0, 0.0, -px]
    sgt = [0.0, 3.0 / hs, 0.0, 3.0, 0.0, -3.0 / hs]
    tiffutil.write_tiff(str(tmp_path / "esa.tif"), esa, gt=egt, compression=8, tile=(1024, 1024))
    tiffutil.write_tiff(str(tmp_path / "soil.tif"), coarse, gt=sgt, compression=5, rows_per_strip=16)
    tiffutil.write_block_shapefile(str(tmp_path / "blocks"), [(1, 0.0, 0.0, 3.0, 3.0)])
    (tmp_path / "config.txt").write_text(
        "hysogs_data_path=%s\nesa_data_path=%s\nblocks_shp_path=%s\nlookup_table_path=%s\nlog_dir=%s\ncog=1\n"
        % (tmp_path / "soil.tif", tmp_path / "esa.tif", tmp_path / "blocks.shp", LOOKUPS, tmp_path / "logs"))
    out = _run(tmp_path, "-c", "config.txt")
    assert out.returncode == 0, out.stderr[-2000:]
    assert "8 levels" in (tmp_path / "logs" / "rank_0.log").read_text()
    xo, yo, W, H, gt = oc.window(egt, size, size, [0.0, 0.0, 3.0, 3.0])
    sxo, syo, hsx, hsy, sg = oc.window(sgt, hs, hs, [0.0, 0.0, 3.0, 3.0])
    soil = coarse[syo:syo + hsy, sxo:sxo + hsx]

    def rows_of(y0, n):
        return oc.process_block_mem(esa[yo + y0:yo + y0 + n, xo:xo + W],
                                    [gt[0], gt[1], 0.0, gt[3] + y0 * gt[5], 0.0, gt[5]], soil, sg, tables)

    y0 = 20000
    want = rows_of(y0, 600)
    ys = np.minimum((np.arange(141) << 8) + 128, H - 1)
    xs = np.minimum((np.arange(141) << 8) + 128, W - 1)
    lvl8 = np.stack([rows_of(int(y), 1)[:, 0, xs] for y in ys], axis=1)      # [18, 141, 141]
    for r in (0, 13, 17):
        c, k = divmod(r, 9)
        p = str(tmp_path / ("cn_rasters_%s" % CONDS[c]) / ("cn_%s_%s_1.tif" % (HCS[k // 3], ARCS[k % 3])))
        cogcheck.check_cog(p, n_levels=8, compression=8)
        with host.Raster(p) as rd:
            np.testing.assert_array_equal(rd.read(0, y0, W, 600), want[r], err_msg=p)
        with Image.open(p) as im:
            im.seek(8)
            np.testing.assert_array_equal(np.array(im), lvl8[r], err_msg=p)
