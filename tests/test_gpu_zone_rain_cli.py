"""GPU: a zonal run under a rainfall raster (bin/gcn10 --zones ... --zone-rain ...) end to end, on the small world of
tests/test_gpu_zonal_cli.py.  The new columns against numpy: the oracle's rasters of each block, masked by the membership
and ownership rules of tests/zoneutil.py and by the cell rule of the raster's grid (include/gcn10_host.h "model grid")
on the block's own pixel centres, summed with the tables of tests/runoffutil.py.  The old columns, as text, against the
run without the raster; a constant raster, as text, against --storm."""
import numpy as np
import pytest

from tests import runoffutil as ru
from tests import tiffutil, zoneutil
from tests.test_gpu_zonal_cli import BLOCKS, PX, ZONES, _run, world  # noqa: F401  (the world and its one plain run)

pytestmark = pytest.mark.gpu

BASE = "zone_id,condition,hc,arc,pixels,valid,sum,mean,min,max,stddev"
NEW = "rain_pixels,rain_mm,rain_valid,runoff_mm_rain,cn_runoff_rain"
UNIT, LAM = 2.5, 0.2
# cells of 37.3 pixels from inside block 7 to inside block 8, above zone 302's lower half: it covers the world partly
ATLAS = dict(xmin=10.0052, ymax=49.9903, dx=37.3 * PX, dy=37.3 * PX, nx=12, ny=8)


def _rows(path, header):
    lines = open(path).read().split("\n")
    assert lines[0] == header and lines[-1] == ""
    return [ln.split(",") for ln in lines[1:-1]]


def _gt(g):
    return [g["xmin"], g["dx"], 0.0, g["ymax"], 0.0, -g["dy"]]


def _cells(g, gt, W, H):
    """(cell column of every pixel column, cell row of every pixel row), -1 = none: ex(k) <= px < ex(k+1) and
    ey(k+1) < py <= ey(k), edges xmin + k dx and ymax - k dy in doubles"""
    px, py = zoneutil.centres(gt, W, H)
    ex = g["xmin"] + np.arange(g["nx"] + 1, dtype=np.float64) * g["dx"]
    ey = g["ymax"] - np.arange(g["ny"] + 1, dtype=np.float64) * g["dy"]
    cx = np.searchsorted(ex, px, side="right") - 1
    cy = np.searchsorted(-ey, -py, side="right") - 1
    return np.where((cx >= 0) & (cx < g["nx"]), cx, -1), np.where((cy >= 0) & (cy < g["ny"]), cy, -1)


def _expected(blocks, g, field, q):
    """per zone record: (rain_pixels, rain_sum, per raster [s, n, sw]) in Python integers"""
    want = [[0, 0, [[0, 0, 0] for _r in range(18)]] for _z in ZONES]
    for _xo, _yo, W, H, gt, bbox, cn in blocks:
        own = zoneutil.own_mask(gt, W, H, bbox)
        cx, cy = _cells(g, gt, W, H)
        inside = (cy >= 0)[:, None] & (cx >= 0)[None, :]
        byte = np.where(inside, field[np.maximum(cy, 0)[:, None], np.maximum(cx, 0)[None, :]], 0).astype(np.int64)
        for zi, (_id, rings) in enumerate(ZONES):
            if rings is None:
                continue
            mask = zoneutil.zone_mask(rings, gt, W, H) & own & inside
            want[zi][0] += int(mask.sum())
            want[zi][1] += int(byte[mask].sum())
            for r in range(18):
                v = cn[r][mask].astype(np.int64)
                ok = v != 255
                t = want[zi][2][r]
                t[0] += int(v[ok].sum())
                t[1] += int(ok.sum())
                t[2] += int(q[byte[mask][ok], v[ok]].sum())
    return want


def _check_new_columns(rows, want, unit, lam):
    it = iter(rows)
    for zi, (_zid, _rings) in enumerate(ZONES):
        pixels, total, triples = want[zi]
        for r in range(18):
            row = next(it)[11:]
            s, n, sw = triples[r]
            assert [int(row[0]), int(row[2])] == [pixels, n], (zi, r, row)
            if pixels == 0:
                assert row[1] == "" and row[3:] == ["", ""], (zi, r, row)
                continue
            mm = (total / pixels) * unit
            assert row[1] == "%.14g" % mm, (zi, r, row)
            if n == 0:
                assert row[3:] == ["", ""], (zi, r, row)
                continue
            assert row[3] == "%.14g" % (sw / n / 100.0), (zi, r, row)
            assert int(row[4]) == ru.cn(s, n, sw, ru.table(mm, lam)), (zi, r, row)


def _config(d, n):
    cfg = (d / "config1.txt").read_text().replace("table1.csv", "table%d.csv" % n).replace("logs1", "logs%d" % n)
    (d / ("config%d.txt" % n)).write_text(cfg)
    return "config%d.txt" % n


def test_a_raster_over_part_of_the_world_equals_the_numpy_oracle(world):  # noqa: F811
    d = world["dir"]
    assert world["run1"].returncode == 0
    field = np.random.default_rng(21).integers(0, 256, (ATLAS["ny"], ATLAS["nx"])).astype(np.uint8)
    field[0, :3] = (0, 255, 0)
    tiffutil.write_tiff(str(d / "atlas.tif"), field, gt=_gt(ATLAS), compression=8, tile=(16, 16))
    out = _run(d, "-c", _config(d, 11), "--zones", "zones.shp", "--zone-rain", "atlas.tif", "--zone-rain-unit", "2.5")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    q = np.stack([ru.table(b * UNIT, LAM) for b in range(256)]).astype(np.int64)
    want = _expected(world["blocks"], ATLAS, field, q)
    # the fixture means something: a zone across both blocks partly under the raster, counted once; zones wholly outside
    plain = world["want"]
    assert 0 < want[0][0] < plain[0][0][0] and want[6][0] == 0 and plain[6][0][0] > 0 and want[4][0] == 0
    in_block = [int((zoneutil.zone_mask(ZONES[0][1], b[4], b[2], b[3]) & zoneutil.own_mask(b[4], b[2], b[3], b[5]) &
                     ((_cells(ATLAS, b[4], b[2], b[3])[1] >= 0)[:, None] &
                      (_cells(ATLAS, b[4], b[2], b[3])[0] >= 0)[None, :])).sum()) for b in world["blocks"]]
    assert min(in_block) > 0 and sum(in_block) == want[0][0]
    rows = _rows(d / "table11.csv", BASE + "," + NEW)
    assert len(rows) == len(ZONES) * 18
    _check_new_columns(rows, want, UNIT, LAM)
    # the columns of the run without the raster, as text
    old = _rows(d / "table1.csv", BASE)
    assert [r[:11] for r in rows] == old
    assert "zone_rain: atlas.tif, 12 x 8 cells" in out.stderr and "zone_rain: depths 0..255 counts" in out.stderr


def test_a_constant_raster_equals_the_storm_columns_as_text(world):  # noqa: F811
    d = world["dir"]
    whole = dict(xmin=9.99, ymax=50.01, dx=0.01, dy=0.01, nx=8, ny=6)
    tiffutil.write_tiff(str(d / "flat.tif"), np.full((6, 8), 20, np.uint8), gt=_gt(whole))
    rain = _run(d, "-c", _config(d, 12), "--zones", "zones.shp", "--zone-rain", "flat.tif", "--zone-rain-unit", "2.5")
    storm = _run(d, "-c", _config(d, 13), "--zones", "zones.shp", "--storm", "50")
    assert rain.returncode == 0 and storm.returncode == 0, rain.stderr[-2000:] + storm.stderr[-2000:]
    a = _rows(d / "table12.csv", BASE + "," + NEW)
    b = _rows(d / "table13.csv", BASE + ",runoff_mm,cn_runoff")
    assert len(a) == len(b) == len(ZONES) * 18
    some = 0
    for ra, rb in zip(a, b):
        assert ra[:11] == rb[:11]
        assert ra[11] == ra[4] and ra[13] == ra[5]                  # every pixel lies under the raster, once
        assert ra[12] == ("50" if int(ra[4]) else "")
        assert ra[14:] == rb[11:], (ra, rb)
        some += ra[14] != ""
    assert some > 18
