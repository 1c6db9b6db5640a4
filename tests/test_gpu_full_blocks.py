"""GPU: bin/gcn10 on full-size blocks of the real VRT geometry (tests/fullblock.py) with the program's own
defaults -- strips of 2304 rows, two workers per GPU on different blocks, GPU inflate of the DEFLATE landcover
through the VRT, the fused DEFLATE encoder with its alias streams -- and every pixel of all 18 rasters of every
block against the reference, in three modes: direct I/O; LZW + COG average + statistics; per-raster encoder + COG
nearest + 4096-row strips + host inflate."""
import multiprocessing
import os
import shutil
import subprocess
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest
from PIL import Image

from gcn10_amd import host
from oracle import cn_oracle_c as oc
from tests import cogcheck
from tests import fullblock as fb
from tests.conftest import LOOKUPS, ROOT
from tests.test_tiff_direct import unaligned_direct_write_refused

pytestmark = pytest.mark.gpu

GCN10 = os.path.join(ROOT, "bin", "gcn10")
CHECKERS = min(6, fb.THREADS)       # processes that decode and compare; each holds a decoded raster (1.3 GB)
_WORLD = {}                         # the world of the module, inherited by the checker processes (fork)


@pytest.fixture(scope="module")
def world(tmp_path_factory, tables):
    wd = str(tmp_path_factory.mktemp("full_blocks"))
    esa, soil = fb.make_world(wd)
    blocks = {}
    for bid, *bbox in fb.BLOCKS:
        xo, yo, W, H, gt = oc.window(fb.VRT_GT, fb.VRT_PX, fb.VRT_PX, bbox)
        sxo, syo, hsx, hsy, sg = oc.window(fb.SOIL_GT, fb.SOIL_PX, fb.SOIL_PX, bbox)
        coarse = np.ascontiguousarray(soil[syo:syo + hsy, sxo:sxo + hsx])
        key = fb.block_keys(esa[yo:yo + H, xo:xo + W], gt, coarse, sg)
        blocks[bid] = dict(xo=xo, yo=yo, W=W, H=H, gt=gt, coarse=coarse, sgt=sg, key=key, khist=fb.key_histogram(key),
                           levels=host.cog_levels(W, H))
    del esa
    a, b, c = (blocks[i] for i in (1, 2, 3))
    # A: one file and a column and a row of its neighbours; B: four files, unaligned to the 1024^2 input tiles;
    # C: a few hundred pixels over the corner of the four files
    assert (a["xo"], a["yo"], a["W"], a["H"]) == (0, 0, 36001, 36001)
    assert (b["W"], b["H"]) == (36001, 36001) and b["xo"] % 1024 and b["yo"] % 1024
    assert b["xo"] < fb.FILE_PX < b["xo"] + b["W"] and b["yo"] < fb.FILE_PX < b["yo"] + b["H"]
    assert c["W"] * c["H"] < 10 ** 6 and c["xo"] < fb.FILE_PX < c["xo"] + c["W"] and c["yo"] < fb.FILE_PX < c["yo"] + c["H"]
    assert a["levels"] == b["levels"] == 8
    _WORLD.update(wd=wd, T=fb.value_table(tables), blocks=blocks)
    yield _WORLD
    _WORLD.clear()
    shutil.rmtree(wd, ignore_errors=True)


def test_reference_equals_the_oracle_on_block_a(world, tables):
    """The table route against oracle_process_block_mem on the first rows, a strip boundary and the last rows of A
    (the last tile row is 161 rows high)."""
    blk, T = world["blocks"][1], world["T"]
    key, gt = blk["key"], blk["gt"]
    for y0, y1 in [(0, 256), (2200, 2400), (blk["H"] - 300, blk["H"])]:
        esa = (key[y0:y1] >> 8).astype(np.uint8)
        want = oc.process_block_mem(esa, [gt[0], gt[1], 0.0, gt[3] + y0 * gt[5], 0.0, gt[5]], blk["coarse"],
                                    blk["sgt"], tables)
        for r in range(18):
            fb.compare(fb.expected_rows(T, key[y0:y1], r), want[r], "A", r, y0)


def test_world_mixes_aliases_and_has_no_two_equal_tiles(world):
    """A tile row of A that crosses the NoData region: tiles equal in all 18 rasters, tiles where only drained ==
    undrained (soil without dual classes), tiles where they differ -- the gather path of the fused encoder.  And
    no two tiles of a raster alike, so that a misplaced tile cannot pass."""
    key, T = world["blocks"][1]["key"], world["T"]
    rows = np.stack([fb.expected_rows(T, key[4096:4352], r) for r in range(18)])
    n = rows.shape[2] // 256
    tiles = rows[:, :, :n * 256].reshape(18, 256, n, 256).transpose(2, 0, 1, 3)        # [tile, raster, y, x]
    all_equal = (tiles == tiles[:, :1]).all(axis=(1, 2, 3))
    dd_equal = (tiles[:, :9] == tiles[:, 9:]).all(axis=(1, 2, 3))
    assert all_equal.sum() >= 4 and (dd_equal & ~all_equal).sum() >= 4 and (~dd_equal).sum() >= 4
    assert len({t.tobytes() for t in tiles[:, 0]}) == n


def _run_mode(world, name, **keys):
    run = os.path.join(world["wd"], name)
    fb.write_config(world["wd"], run, LOOKUPS, **keys)
    out = subprocess.run([GCN10, "-c", "config.txt", "--gpus", "1"], cwd=run, capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    logs = sorted(f for f in os.listdir(os.path.join(run, "logs")) if f.startswith("rank_"))
    text = {f: open(os.path.join(run, "logs", f)).read() for f in logs}
    errors = [line for t in text.values() for line in t.splitlines() if "ERROR" in line]
    assert not errors, errors[:5]
    assert "starting processing with 2 gpu workers" in text["rank_0.log"]
    parts = [os.path.join(d, f) for d, _s, fs in os.walk(run) for f in fs if f.endswith(".part")]
    assert not parts, parts[:5]
    missing = [fb.raster_name(r, bid) for bid in world["blocks"] for r in range(18)
               if not os.path.exists(os.path.join(run, fb.raster_name(r, bid)))]
    assert not missing, missing
    return run, text


def _check_one(job):
    path, bid, r, strip_rows, resampling, compression = job
    blk = _WORLD["blocks"][bid]
    try:
        with Image.open(path) as im:
            assert im.tag_v2[259] == compression, "%s: compression %s" % (path, im.tag_v2[259])
        if resampling:
            cogcheck.check_cog(path, n_levels=blk["levels"], compression=compression)
        fb.check_raster(path, _WORLD["T"], blk["key"], "ABC"[bid - 1], r, strip_rows, resampling,
                        blk["levels"] if resampling else 0, blk.get("nearest"), band=2048)
    except AssertionError as e:
        return str(e)
    return None


def _check_all(world, run, strip_rows=fb.DEFAULT_STRIP_ROWS, resampling=None, compression=8):
    jobs = [(os.path.join(run, fb.raster_name(r, bid)), bid, r, strip_rows, resampling, compression)
            for bid in sorted(world["blocks"], key=lambda b: -world["blocks"][b]["W"]) for r in range(18)]
    with ProcessPoolExecutor(CHECKERS, mp_context=multiprocessing.get_context("fork")) as ex:
        errors = [e for e in ex.map(_check_one, jobs) if e]
    assert not errors, "%d of %d files differ:\n%s" % (len(errors), len(jobs), "\n".join(errors[:8]))


def test_mode1_direct_io(world):
    run, _log = _run_mode(world, "mode1", direct_io=1)
    try:
        print("\noutput file system refuses unaligned O_DIRECT writes: %s" % unaligned_direct_write_refused(run))
        _check_all(world, run)
    finally:
        shutil.rmtree(run, ignore_errors=True)


def test_mode2_lzw_cog_average_stats(world):
    run, log = _run_mode(world, "mode2", compress="lzw", cog=1, overview_resampling="average", stats=1, nodata=255)
    try:
        assert "8 levels" in "".join(log.values())
        _check_all(world, run, resampling="average", compression=5)
        T = world["T"]
        for bid, blk in world["blocks"].items():
            for r in range(18):
                # the tags against the statistics of the EXPECTED raster, not of what was decoded
                fb.check_tags(os.path.join(run, fb.raster_name(r, bid)), fb.raster_histogram(T, blk["khist"], r), 255)
    finally:
        shutil.rmtree(run, ignore_errors=True)


def test_mode3_per_raster_encoder_nearest_largest_strips_host_inflate(world):
    for blk in world["blocks"].values():
        blk["nearest"] = [fb.nearest_level(blk["key"], k) for k in range(1, blk["levels"] + 1)]
    run, log = _run_mode(world, "mode3", gpu_deflate=1, cog=1, strip_rows=4096, gpu_inflate=0)
    try:
        assert "8 levels" in "".join(log.values())
        _check_all(world, run, strip_rows=4096, resampling="nearest")
    finally:
        shutil.rmtree(run, ignore_errors=True)
        for blk in world["blocks"].values():
            blk.pop("nearest", None)
