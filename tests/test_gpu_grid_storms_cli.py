"""GPU: several design storms end to end.  The two-block world of tests/test_gpu_grid_cli.py (its fixture and helpers),
and what `bin/gcn10 --grid ... --storms 25:50:100` writes under cn_grid_<cond>/: the mean rasters, byte for byte those of
the run without a storm, and cnq_<hc>_<arc>_p2500 / _p5000 / _p10000.tif beside each, the _p5000 ones byte for byte
what `--storm 50` alone writes.  `--storms 50` against `--storm 50`, file by file.  Then the zone fixture of
tests/test_gpu_zonal_cli.py with the same storms: the table's six more columns.

Expected: the oracle's process_block_mem rasters of each block, masked by the ownership rule, accumulated over both
blocks with one more word per storm (tests/stormutil.py), then the cell rule in numpy per storm."""
import os

import numpy as np
import pytest

from tests import gridutil as gu
from tests import runoffutil as ru
from tests import stormutil as su
from tests import zoneutil
from tests.test_gpu_grid_cli import (ARCS, CONDS, GRID, GRID_TEXT, HCS, NX, NY, _config, _name, _read, _run,  # noqa: F401
                                     world)
from tests.test_gpu_zonal_cli import ZONES, _check_rows, _rows
from tests.test_gpu_zonal_cli import _run as _run_zonal
from tests.test_gpu_zonal_cli import world as zonal_world  # noqa: F401

pytestmark = pytest.mark.gpu

STORMS = "25:50:100"
DEPTHS = (25, 50, 100)
QS = np.stack([ru.table(p, 0.2) for p in DEPTHS])
SUFFIXES = ("_p2500", "_p5000", "_p10000")
HEADER = "zone_id,condition,hc,arc,pixels,valid,sum,mean,min,max,stddev"


def _qname(r, suffix):
    c, k = divmod(r, 9)
    return os.path.join("cn_grid_%s" % CONDS[c], "cnq_%s_%s%s.tif" % (HCS[k // 3], ARCS[k % 3], suffix))


def _words(world, bids):  # noqa: F811
    """int64[18][NY][NX][5] = {s, n, sw of 25, 50, 100 mm} over the owned pixels of the blocks"""
    acc = np.zeros((18, NY, NX, 5), np.int64)
    for bid in bids:
        b = world["blocks"][bid]
        kx, ky = gu.cells(GRID, b["gt"], b["W"], b["H"])
        m = zoneutil.own_mask(b["gt"], b["W"], b["H"], b["bbox"])
        kx, ky = np.where(m.any(axis=0), kx, -1), np.where(m.any(axis=1), ky, -1)
        for r in range(18):
            su.add_words(acc[r], b["cn"][r], kx, ky, QS)
    return acc


def _files(run_dir):
    return sorted(os.path.join(sub, f) for sub in os.listdir(run_dir) if sub.startswith("cn_")
                  for f in os.listdir(run_dir / sub))


@pytest.fixture(scope="module")
def storms(world):  # noqa: F811
    d = world["dir"]
    run = _config(d, "storms")
    out = _run(run, "-c", "config.txt", "--grid", GRID_TEXT, "--storms", STORMS)
    one = _config(d, "storm50")
    out50 = _run(one, "-c", "config.txt", "--grid", GRID_TEXT, "--storm", "50")
    return {"dir": run, "out": out, "dir50": one, "out50": out50, "acc": _words(world, (7, 8))}


def test_the_world_holds_every_kind_of_cell(world, storms):  # noqa: F811
    """From the expected words alone (no GPU work): cells without a valid pixel, cells that shed nothing in the smallest
    storm only, and cells that shed in all three."""
    acc = storms["acc"]
    np.testing.assert_array_equal(acc[..., :2], world["both"])          # words 0 and 1 are the mean run's
    n = acc[..., 1]
    assert [int(q[100]) for q in QS] == [2500, 5000, 10000]
    assert (n == 0).any()
    assert ((n > 0) & (acc[..., 2] == 0) & (acc[..., 3] > 0) & (acc[..., 4] > 0)).any()
    assert ((acc[..., 2] > 0) & (acc[..., 3] > 0) & (acc[..., 4] > 0)).any()
    assert (acc[..., 2] <= acc[..., 3]).all() and (acc[..., 3] <= acc[..., 4]).all()
    cnq = su.cn_arrays(acc, QS)
    assert (cnq[0] != cnq[1]).any() and (cnq[1] != cnq[2]).any()        # the three rasters differ


def _check_storm_files(run_dir, acc):
    want = su.cn_arrays(acc, QS)
    for r in range(18):
        mean_tags, _mean = _read(str(run_dir / _name(r)))
        for j, suffix in enumerate(SUFFIXES):
            path = str(run_dir / _qname(r, suffix))
            tags, got = _read(path)
            assert (tags[256], tags[257]) == (NX, NY), path
            assert tuple(tags[33550]) == (GRID["dx"], GRID["dy"], 0.0), path                        # ModelPixelScale
            assert tuple(tags[33922]) == (0.0, 0.0, 0.0, GRID["xmin"], GRID["ymax"], 0.0), path     # ModelTiepoint
            assert 34735 in tags and tags[34735] == mean_tags[34735] and 42113 not in tags, path
            bad = np.argwhere(got != want[j][r])
            assert bad.size == 0, "%s: %d cells differ, first %s: got %d, want %d" % (
                path, len(bad), bad[0], got[tuple(bad[0])], want[j][r][tuple(bad[0])])
    files = _files(run_dir)
    assert len(files) == 18 * 4 and not [f for f in files if ".part" in f]
    for suffix in SUFFIXES:
        assert len([f for f in files if "cnq_" in f and f.endswith(suffix + ".tif")]) == 18


def test_three_storms_in_one_run(world, storms):  # noqa: F811
    out, d = storms["out"], storms["dir"]
    assert world["base"].returncode == 0 and out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    for r in range(18):     # the means: the bytes of the run without a storm
        assert (d / _name(r)).read_bytes() == (world["dir"] / "base" / _name(r)).read_bytes(), _name(r)
    _check_storm_files(d, storms["acc"])
    text = out.stdout + out.stderr
    lines = [ln for ln in text.split("\n") if "storm: P = " in ln]
    assert len(lines) == 3                                  # one line per storm, in the order given
    for ln, (p, t) in zip(lines, ((25, ru.threshold(QS[0])), (50, 51), (100, ru.threshold(QS[2])))):
        assert "storm: P = %d mm, lambda = 0.20000000000000001, threshold CN %d " % (p, t) in ln, ln
    assert ("under cn_grid_<cond>/: cn_<hc>_<arc>.tif (mean) and cnq_<hc>_<arc>_p2500.tif, _p5000.tif, _p10000.tif "
            "(runoff-equivalent)") in text
    log = "".join((d / "logs" / f).read_text() for f in os.listdir(d / "logs"))
    assert "ERROR" not in log and log.count("storm: P = ") == 3


def test_every_storm_is_the_file_of_its_own_run(world, storms):  # noqa: F811
    assert storms["out50"].returncode == 0, storms["out50"].stderr[-2000:]
    for r in range(18):
        name = _qname(r, "_p5000")
        assert (storms["dir"] / name).read_bytes() == (storms["dir50"] / name).read_bytes(), name
    # and with a ratio of its own: 25 mm at lambda 0.05 from a ladder and alone
    d = world["dir"]
    a, b = _config(d, "storms_ratio"), _config(d, "storm_ratio")
    out = _run(a, "-c", "config.txt", "--grid", GRID_TEXT, "--storms", "25:100,0.05", "--lookups", "g_ii")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    out = _run(b, "-c", "config.txt", "--grid", GRID_TEXT, "--storm", "25,0.05", "--lookups", "g_ii")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    mine = [f for f in _files(b) if "cnq_" in f]
    assert len(mine) == 2 and all(f.endswith("_p2500.tif") for f in mine)
    assert len(_files(a)) == 6
    for f in _files(b):
        assert (a / f).read_bytes() == (b / f).read_bytes(), f


def test_one_depth_is_the_storm_run_byte_for_byte(world, storms):  # noqa: F811
    d = world["dir"]
    one = _config(d, "storms_one")
    out = _run(one, "-c", "config.txt", "--grid", GRID_TEXT, "--storms", "50")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert _files(one) == _files(storms["dir50"]) and len(_files(one)) == 36
    for f in _files(one):
        assert (one / f).read_bytes() == (storms["dir50"] / f).read_bytes(), f

    def lines(o):
        return [ln.split("[rank 0] ", 1)[-1] for ln in (o.stdout + o.stderr).split("\n") if "storm: " in ln or "grid: " in ln]
    assert lines(out) == lines(storms["out50"]) and len(lines(out)) == 2


def test_block_order_and_workers_do_not_change_a_byte(world, storms):  # noqa: F811
    d = world["dir"]
    rev = _config(d, "storms_reversed")
    (rev / "blocks.txt").write_text("8\n7\n")
    out = _run(rev, "-c", "config.txt", "-l", "blocks.txt", "--grid", GRID_TEXT, "--storms", STORMS + ",0.2")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    two = _config(d, "storms_two", extra="grid=%s\nstorms=%s\n" % (GRID_TEXT, STORMS))     # the keys instead of the flags
    out = _run(two, "-c", "config.txt", "--gpus", "2", env={"GCN10_OVERSUBSCRIBE": "1"})
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    for run in (rev, two):
        assert _files(run) == _files(storms["dir"])
        for f in _files(run):
            assert (run / f).read_bytes() == (storms["dir"] / f).read_bytes(), f


# ---- the zonal table --------------------------------------------------------------------------------------------

def _zone_runoff(blocks, zones):
    """per zone record and raster: [valid, sum, sum of q[v] per storm] in Python integers"""
    want = [[[0, 0, 0, 0, 0] for _r in range(18)] for _z in zones]
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
                for j in range(3):
                    want[zi][r][2 + j] += int(QS[j].astype(np.int64)[ok].sum())
    return want


def test_the_zonal_table_gets_six_columns(zonal_world):  # noqa: F811
    d = zonal_world["dir"]
    assert zonal_world["run1"].returncode == 0
    before = (d / "table1.csv").read_bytes()
    _rows(d / "table1.csv")                                 # without a storm: today's header, asserted there
    cfg = (d / "config1.txt").read_text().replace("table1.csv", "table7.csv").replace("logs1", "logs7")
    (d / "config7.txt").write_text(cfg)
    out = _run_zonal(d, "-c", "config7.txt", "--zones", "zones.shp", "--storms", STORMS)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = (d / "table7.csv").read_text().split("\n")
    assert lines[0] == HEADER + "".join(",runoff_mm%s,cn_runoff%s" % (s, s) for s in SUFFIXES)
    assert lines[-1] == ""
    rows = [ln.split(",") for ln in lines[1:-1]]
    assert all(len(row) == 17 for row in rows)
    # the first eleven fields are the bytes of the table without a storm
    assert ("\n".join(",".join(row[:11]) for row in [lines[0].split(",")] + rows) + "\n").encode() == before
    _check_rows([row[:11] for row in rows], zonal_world["want"], range(18))
    want = _zone_runoff(zonal_world["blocks"], ZONES)
    it = iter(rows)
    seen = set()
    for zi in range(len(ZONES)):
        for r in range(18):
            row = next(it)
            valid, total = want[zi][r][:2]
            assert int(row[5]) == valid and int(row[6]) == total
            if valid == 0:
                assert row[11:] == [""] * 6, row
                seen.add("empty")
                continue
            for j in range(3):
                sw = want[zi][r][2 + j]
                assert row[11 + 2 * j] == "%.14g" % (sw / valid / 100.0), row
                assert int(row[12 + 2 * j]) == ru.cn(total, valid, sw, QS[j]), row
            seen.add("differ" if len({row[12], row[14], row[16]}) > 1 else "same")
    assert seen >= {"empty", "differ"}, seen             # zones without a valid pixel; composites that depend on the storm
    # one depth, from the key: the table of --storm 50, byte for byte, plain column names
    for n, extra in ((8, "storms=50\n"), (9, "storm=50\n")):
        (d / ("config%d.txt" % n)).write_text(cfg.replace("table7.csv", "table%d.csv" % n).replace("logs7", "logs%d" % n)
                                              + extra + "zonal=1\nzones_shp_path=zones.shp\n")
        out = _run_zonal(d, "-c", "config%d.txt" % n)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert (d / "table8.csv").read_bytes() == (d / "table9.csv").read_bytes()
    assert (d / "table8.csv").read_text().split("\n")[0] == HEADER + ",runoff_mm,cn_runoff"
    # and its two columns are the 50 mm columns of the ladder
    rows50 = [ln.split(",") for ln in (d / "table8.csv").read_text().split("\n")[1:-1]]
    assert [row[11:13] for row in rows50] == [row[13:15] for row in rows]
