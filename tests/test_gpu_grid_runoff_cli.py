"""GPU: a design storm end to end.  The two-block world of tests/test_gpu_grid_cli.py (its fixture and helpers), and
what `bin/gcn10 --grid ... --storm 50` writes under cn_grid_<cond>/: the mean rasters, byte for byte those of the run
without a storm, and cnq_<hc>_<arc>_p5000.tif beside each.  Then the zone fixture of tests/test_gpu_zonal_cli.py with
the same storm: the table's two more columns.

Expected: the oracle's process_block_mem rasters of each block, masked by the ownership rule, accumulated over both
blocks with one more word for q[v] (tests/runoffutil.py), then the cell rule in numpy.  50 mm (lambda 0.2, threshold CN
51) gives every kind of cell the first test asks for, so that is the storm."""
import os

import numpy as np
import pytest

from tests import gridutil as gu
from tests import runoffutil as ru
from tests import zoneutil
from tests.test_gpu_grid_cli import (ARCS, CONDS, GRID, GRID_TEXT, HCS, NX, NY, _config, _name, _read, _run,  # noqa: F401
                                     world)
from tests.test_gpu_zonal_cli import ZONES, _check_rows, _rows
from tests.test_gpu_zonal_cli import _run as _run_zonal
from tests.test_gpu_zonal_cli import world as zonal_world  # noqa: F401

pytestmark = pytest.mark.gpu

STORM = "50"
Q = ru.table(50, 0.2)
SUFFIX = "_p5000"


def _qname(r):
    c, k = divmod(r, 9)
    return os.path.join("cn_grid_%s" % CONDS[c], "cnq_%s_%s%s.tif" % (HCS[k // 3], ARCS[k % 3], SUFFIX))


def _triples(world, bids):  # noqa: F811
    """int64[18][NY][NX][3] = {s, n, sw} over the owned pixels of the blocks, and the blocks that feed every cell"""
    acc = np.zeros((18, NY, NX, 3), np.int64)
    fed = np.zeros((NY, NX), np.int64)
    for bid in bids:
        b = world["blocks"][bid]
        kx, ky = gu.cells(GRID, b["gt"], b["W"], b["H"])
        m = zoneutil.own_mask(b["gt"], b["W"], b["H"], b["bbox"])
        kx, ky = np.where(m.any(axis=0), kx, -1), np.where(m.any(axis=1), ky, -1)
        for r in range(18):
            ru.add_triples(acc[r], b["cn"][r], kx, ky, Q)
        count = np.zeros((NY, NX, 2), np.int64)
        gu.add_sums(count, np.zeros((b["H"], b["W"]), np.uint8), kx, ky)
        fed += count[..., 1] > 0
    return acc, fed


@pytest.fixture(scope="module")
def storm(world):  # noqa: F811
    d = world["dir"]
    run = _config(d, "storm")
    out = _run(run, "-c", "config.txt", "--grid", GRID_TEXT, "--storm", STORM)
    acc, fed = _triples(world, (7, 8))
    return {"dir": run, "out": out, "acc": acc, "fed": fed}


def test_the_world_holds_every_kind_of_cell(world, storm):  # noqa: F811
    """From the expected triples alone (no GPU work): among the cells fed by both blocks and among the others, cells
    where no pixel sheds water, cells that shed some and cells whose composite lies above their mean; and cells without a
    valid pixel -- among the others only: this world's seam column holds valid pixels in every cell and raster, and the
    count does not depend on the storm, so no P gives a cell of both blocks with n = 0.  The rule's n = 0 branch for
    sums merged on the host is gcn10_runoff_cn's, held by tests/test_runoff_host.py."""
    acc, fed = storm["acc"], storm["fed"]
    np.testing.assert_array_equal(acc[..., :2], world["both"])          # words 0 and 1 are the mean run's
    n, sw = acc[..., 1], acc[..., 2]
    cnq, mean = ru.cn_array(acc, Q), gu.means(acc[..., :2])
    assert ru.threshold(Q) == 51 and int(Q[100]) == 5000
    for where in (fed == 2, fed == 1):
        assert where.any()
        w = np.broadcast_to(where[None], n.shape)
        assert (w & (n > 0) & (sw == 0)).any()
        assert (w & (sw > 0)).any()
        assert (w & (sw > 0) & (cnq > mean)).any()
    assert (np.broadcast_to((fed == 1)[None], n.shape) & (n == 0)).any()
    assert (fed == 0).any() and (n[:, fed == 0] == 0).all()        # cells no block feeds
    assert not ((sw > 0) & (cnq < mean)).any()              # Q(CN) is convex: the composite never lies below the mean


def test_the_mean_rasters_are_the_bytes_of_the_run_without_a_storm(world, storm):  # noqa: F811
    out, d = storm["out"], storm["dir"]
    assert world["base"].returncode == 0 and out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    for r in range(18):
        assert (d / _name(r)).read_bytes() == (world["dir"] / "base" / _name(r)).read_bytes(), _name(r)


def _check_storm_files(run_dir, acc, nodata):
    want = ru.cn_array(acc, Q)
    for r in range(18):
        path = str(run_dir / _qname(r))
        tags, got = _read(path)
        mean_tags, _mean = _read(str(run_dir / _name(r)))
        # what tests/test_gpu_grid_cli.py::_check_files asserts for the mean files
        assert (tags[256], tags[257]) == (NX, NY), path
        assert (tags[322], tags[323]) == (256, 256) and tags[258] == (8,) and tags[259] == 8 and len(tags[324]) == 1, path
        assert tuple(tags[33550]) == (GRID["dx"], GRID["dy"], 0.0), path                            # ModelPixelScale
        assert tuple(tags[33922]) == (0.0, 0.0, 0.0, GRID["xmin"], GRID["ymax"], 0.0), path         # ModelTiepoint
        assert 34735 in tags and tags[34735] == mean_tags[34735], path          # the landcover's geo keys
        assert 42112 not in tags, path
        if nodata is None:
            assert 42113 not in tags, path
        else:
            assert tags[42113] == str(nodata), path
        bad = np.argwhere(got != want[r])
        assert bad.size == 0, "%s: %d cells differ, first %s: got %d, want %d" % (
            path, len(bad), bad[0], got[tuple(bad[0])], want[r][tuple(bad[0])])
    dirs = sorted(f for f in os.listdir(run_dir) if f.startswith("cn_"))
    assert dirs == ["cn_grid_drained", "cn_grid_undrained"]
    for sub in dirs:
        files = sorted(os.listdir(run_dir / sub))
        assert len(files) == 18 and not [f for f in files if ".part" in f]
        assert len([f for f in files if f.startswith("cnq_") and f.endswith(SUFFIX + ".tif")]) == 9


def test_the_runoff_equivalent_rasters_of_both_blocks(world, storm):  # noqa: F811
    out, d = storm["out"], storm["dir"]
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    _check_storm_files(d, storm["acc"], None)
    text = out.stdout + out.stderr
    assert "storm: P = 50 mm, lambda = 0.20000000000000001, threshold CN 51" in text
    assert ("under cn_grid_<cond>/: cn_<hc>_<arc>.tif (mean) and cnq_<hc>_<arc>_p5000.tif (runoff-equivalent)"
            in text)
    log = "".join((d / "logs" / f).read_text() for f in os.listdir(d / "logs"))
    assert "ERROR" not in log and "threshold CN 51" in log


def test_block_order_and_workers_do_not_change_a_byte(world, storm):  # noqa: F811
    d = world["dir"]
    rev = _config(d, "storm_reversed")
    (rev / "blocks.txt").write_text("8\n7\n")
    out = _run(rev, "-c", "config.txt", "-l", "blocks.txt", "--grid", GRID_TEXT, "--storm", "50,0.2")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    two = _config(d, "storm_two", extra="grid=%s\nstorm=%s\n" % (GRID_TEXT, STORM))     # the keys instead of the flags
    out = _run(two, "-c", "config.txt", "--gpus", "2", env={"GCN10_OVERSUBSCRIBE": "1"})
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    for run in (rev, two):
        _check_storm_files(run, storm["acc"], None)
        for r in range(18):
            for name in (_name(r), _qname(r)):
                assert (run / name).read_bytes() == (storm["dir"] / name).read_bytes(), name
    # both at once and a NoData tag: the tag in both files of every raster, not a cell changed
    tagged = _config(d, "storm_tagged", extra="nodata=255\n")
    (tagged / "blocks.txt").write_text("8\n7\n")
    out = _run(tagged, "-c", "config.txt", "-l", "blocks.txt", "--grid", GRID_TEXT, "--storm", STORM, "--gpus", "2",
               env={"GCN10_OVERSUBSCRIBE": "1"})
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    _check_storm_files(tagged, storm["acc"], 255)
    for r in range(18):
        tags, got = _read(str(tagged / _name(r)))
        assert tags[42113] == "255"
        np.testing.assert_array_equal(got, _read(str(storm["dir"] / _name(r)))[1])


# ---- the zonal table --------------------------------------------------------------------------------------------

def _zone_runoff(blocks, zones):
    """per zone record and raster: [valid, sum, sum of q[v]] in Python integers"""
    want = [[[0, 0, 0] for _r in range(18)] for _z in zones]
    for _xo, _yo, W, H, gt, bbox, cn in blocks:
        own = zoneutil.own_mask(gt, W, H, bbox)
        for zi, (_id, rings) in enumerate(zones):
            if rings is None:
                continue
            mask = zoneutil.zone_mask(rings, gt, W, H) & own
            for r in range(18):
                v = cn[r][mask].astype(np.int64)
                ok = v[v != 255]
                want[zi][r][0] += int(ok.size)
                want[zi][r][1] += int(ok.sum())
                want[zi][r][2] += int(Q.astype(np.int64)[ok].sum())
    return want


def test_the_zonal_table_gets_two_columns(zonal_world):  # noqa: F811
    d = zonal_world["dir"]
    assert zonal_world["run1"].returncode == 0
    before = (d / "table1.csv").read_bytes()
    _rows(d / "table1.csv")                                 # without a storm: today's header, asserted there
    cfg = (d / "config1.txt").read_text().replace("table1.csv", "table5.csv").replace("logs1", "logs5")
    (d / "config5.txt").write_text(cfg)
    out = _run_zonal(d, "-c", "config5.txt", "--zones", "zones.shp", "--storm", STORM)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = (d / "table5.csv").read_text().split("\n")
    assert lines[0] == "zone_id,condition,hc,arc,pixels,valid,sum,mean,min,max,stddev,runoff_mm,cn_runoff"
    assert lines[-1] == ""
    rows = [ln.split(",") for ln in lines[1:-1]]
    assert all(len(row) == 13 for row in rows)
    # the first eleven fields are the bytes of the table without a storm
    assert ("\n".join(",".join(row[:11]) for row in [lines[0].split(",")] + rows) + "\n").encode() == before
    _check_rows([row[:11] for row in rows], zonal_world["want"], range(18))
    want = _zone_runoff(zonal_world["blocks"], ZONES)
    it = iter(rows)
    seen = set()
    for zi in range(len(ZONES)):
        for r in range(18):
            row = next(it)
            valid, total, sw = want[zi][r]
            assert int(row[5]) == valid and int(row[6]) == total
            if valid == 0:
                assert row[11:] == ["", ""], row
                seen.add("empty")
                continue
            assert row[11] == "%.14g" % (sw / valid / 100.0), row
            assert int(row[12]) == ru.cn(total, valid, sw, Q), row
            seen.add("dry" if sw == 0 else "above" if int(row[12]) > (2 * total + valid) // (2 * valid) else "wet")
    assert seen >= {"empty", "above"}, seen             # zones without a valid pixel, zones whose composite beats the mean
    # the same storm from the config key, with a ratio: the same table for the default ratio
    (d / "config6.txt").write_text(cfg.replace("table5.csv", "table6.csv").replace("logs5", "logs6")
                                   + "storm=50,0.2\nzonal=1\nzones_shp_path=zones.shp\n")
    out = _run_zonal(d, "-c", "config6.txt")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert (d / "table6.csv").read_bytes() == (d / "table5.csv").read_bytes()
