"""GPU: a rainfall raster on the model grid end to end.  The two-block world of tests/test_gpu_grid_cli.py (its fixture
and helpers), rain rasters written with tests/tiffutil.py, and what `bin/gcn10 --grid ... --rain <file>` writes under
cn_grid_<cond>/: the mean rasters, byte for byte those of the run without rain, and cnq_<hc>_<arc>_rain.tif beside each.

Expected: the oracle's process_block_mem rasters of each block, masked by the ownership rule, accumulated over both blocks
per cell with the table of the cell's own byte, then runoffutil.cn per cell (tests/rainutil.py); a constant field of 50
against what `--storm 50` writes."""
import os

import numpy as np
import pytest

from tests import gridutil as gu
from tests import rainutil as rn
from tests import runoffutil as ru
from tests import tiffutil, zoneutil
from tests.test_gpu_grid_cli import (ARCS, CONDS, GRID, GRID_TEXT, HCS, NX, NY, _config, _name, _read, _run,  # noqa: F401
                                     world)

pytestmark = pytest.mark.gpu

GT = [GRID["xmin"], GRID["dx"], 0.0, GRID["ymax"], 0.0, -GRID["dy"]]
UNIT, LAMBDA = 2.5, 0.05


def _qname(r, suffix="_rain"):
    c, k = divmod(r, 9)
    return os.path.join("cn_grid_%s" % CONDS[c], "cnq_%s_%s%s.tif" % (HCS[k // 3], ARCS[k % 3], suffix))


def _files(run_dir):
    return sorted(os.path.join(sub, f) for sub in os.listdir(run_dir) if sub.startswith("cn_")
                  for f in os.listdir(run_dir / sub))


def _triples(world, field, tables):  # noqa: F811
    """int64[18][NY][NX][3] over the owned pixels of both blocks"""
    acc = np.zeros((18, NY, NX, 3), np.int64)
    for bid in (7, 8):
        b = world["blocks"][bid]
        kx, ky = gu.cells(GRID, b["gt"], b["W"], b["H"])
        m = zoneutil.own_mask(b["gt"], b["W"], b["H"], b["bbox"])
        kx, ky = np.where(m.any(axis=0), kx, -1), np.where(m.any(axis=1), ky, -1)
        for r in range(18):
            rn.add_triples(acc[r], b["cn"][r], kx, ky, field, tables)
    return acc


@pytest.fixture(scope="module")
def fields(world):  # noqa: F811
    d = world["dir"]
    rng = np.random.default_rng(21)
    random = rng.integers(0, 256, (NY, NX)).astype(np.uint8)
    random.reshape(-1)[rng.permutation(NX * NY)[:256]] = np.arange(256, dtype=np.uint8)       # every byte is there
    f = {"random": random, "fifty": np.full((NY, NX), 50, np.uint8), "dry": np.zeros((NY, NX), np.uint8)}
    tiffutil.write_tiff(str(d / "random.tif"), f["random"], gt=GT, compression=8, tile=(16, 16))
    tiffutil.write_tiff(str(d / "fifty.tif"), f["fifty"], gt=GT)
    tiffutil.write_tiff(str(d / "dry.tif"), f["dry"])                                         # without georeferencing
    return f


def test_a_constant_field_of_50_is_the_storm_of_50_mm(world, fields):  # noqa: F811
    d = world["dir"]
    run, storm = _config(d, "rain_fifty"), _config(d, "rain_storm50")
    out = _run(run, "-c", "config.txt", "--grid", GRID_TEXT, "--rain", str(d / "fifty.tif"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    out50 = _run(storm, "-c", "config.txt", "--grid", GRID_TEXT, "--storm", "50")
    assert world["base"].returncode == 0 and out50.returncode == 0, out50.stdout[-2000:] + out50.stderr[-2000:]
    for r in range(18):
        assert (run / _name(r)).read_bytes() == (d / "base" / _name(r)).read_bytes(), _name(r)
        tags, got = _read(str(run / _qname(r)))
        tags50, want = _read(str(storm / _qname(r, "_p5000")))
        np.testing.assert_array_equal(got, want, err_msg=_qname(r))
        assert tags[33550] == tags50[33550] and tags[33922] == tags50[33922] and tags[34735] == tags50[34735]
    files = _files(run)
    assert len(files) == 36 and len([f for f in files if f.endswith("_rain.tif")]) == 18
    assert not [f for f in files if ".part" in f]
    text = out.stdout + out.stderr
    assert "rain: %s, %d x %d cells, unit = 1 mm, lambda = 0.20000000000000001" % (d / "fifty.tif", NX, NY) in text
    assert "rain: depths 50..50 counts, 0 cells without rain" in text
    assert "under cn_grid_<cond>/: cn_<hc>_<arc>.tif (mean) and cnq_<hc>_<arc>_rain.tif (runoff-equivalent)" in text
    log = "".join((run / "logs" / f).read_text() for f in os.listdir(run / "logs"))
    assert "ERROR" not in log and log.count("rain: depths ") == 1


def test_a_random_field_astride_two_blocks_equals_the_restatement(world, fields):  # noqa: F811
    """Cell column 13 lies astride the seam of blocks 7 and 8: its cells are shared and finished on the host with the
    table of their own byte; the others become bytes on the device."""
    d = world["dir"]
    run = _config(d, "rain_random")
    out = _run(run, "-c", "config.txt", "--grid", GRID_TEXT, "--rain", str(d / "random.tif"), "--rain-unit",
               "%r,%r" % (UNIT, LAMBDA))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    tables = np.stack([ru.table(b * UNIT, LAMBDA) for b in range(256)])
    acc = _triples(world, fields["random"], tables)
    np.testing.assert_array_equal(acc[..., :2], world["both"])
    assert "shared with other blocks" in "".join((run / "logs" / f).read_text() for f in os.listdir(run / "logs"))
    n, sw = acc[..., 1], acc[..., 2]
    assert (n == 0).any() and ((n > 0) & (sw == 0)).any() and (sw > 0).any()
    for r in range(18):
        assert (run / _name(r)).read_bytes() == (d / "base" / _name(r)).read_bytes(), _name(r)
        want = rn.cn_cells(acc[r].reshape(1, -1, 3), fields["random"], tables).reshape(NY, NX)
        _tags, got = _read(str(run / _qname(r)))
        bad = np.argwhere(got != want)
        assert bad.size == 0, "%s: %d cells differ, first %s: got %d, want %d" % (
            _qname(r), len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    text = out.stdout + out.stderr
    assert "unit = 2.5 mm, lambda = 0.050000000000000003" in text
    assert "rain: depths 0..255 counts, %d cells without rain" % int((fields["random"] == 0).sum()) in text
    # other worker counts, the other block order, the keys instead of the flags: the same bytes
    rev = _config(d, "rain_reversed")
    (rev / "blocks.txt").write_text("8\n7\n")
    out = _run(rev, "-c", "config.txt", "-l", "blocks.txt", "--grid", GRID_TEXT, "--rain", str(d / "random.tif"),
               "--rain-unit", "%r,%r" % (UNIT, LAMBDA), "--gpus", "1", env={"GCN10_OVERSUBSCRIBE": "1"})
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    two = _config(d, "rain_two", extra="grid=%s\nrain=%s\nrain_unit=%r,%r\n" % (GRID_TEXT, d / "random.tif", UNIT, LAMBDA))
    out = _run(two, "-c", "config.txt", "--gpus", "2", env={"GCN10_OVERSUBSCRIBE": "1"})
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    for other in (rev, two):
        assert _files(other) == _files(run) and len(_files(run)) == 36
        for f in _files(other):
            assert (other / f).read_bytes() == (run / f).read_bytes(), f


def test_a_field_of_zeros_gives_the_means(world, fields):  # noqa: F811
    d = world["dir"]
    run = _config(d, "rain_dry")
    out = _run(run, "-c", "config.txt", "--grid", GRID_TEXT, "--rain", str(d / "dry.tif"), "--lookups", "g_ii,p_i")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    files = _files(run)
    assert len(files) == 8
    for f in files:
        if "cnq_" in f:
            _tags, got = _read(str(run / f))
            _tags, mean = _read(str(run / f.replace("cnq_", "cn_").replace("_rain.tif", ".tif")))
            np.testing.assert_array_equal(got, mean, err_msg=f)
    assert "rain: depths 0..0 counts, %d cells without rain" % (NX * NY) in out.stdout + out.stderr
