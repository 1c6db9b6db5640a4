"""GPU: the zonal run mode end to end.  A small world -- DEFLATE landcover in 256^2 tiles at the real pixel size, LZW
soil 25 times coarser, two adjacent blocks whose windows share a pixel column -- and a zone file; the table
`bin/gcn10 --zones` writes against the oracle's 18 rasters of each block, masked by the numpy membership and ownership
rules of tests/zoneutil.py; and a second zone file, a triangulated lattice on pixel centres across both blocks."""
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import cn_oracle_c as oc
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
ZONES = [
    (301, [[(10.0113, 49.9951), (10.0447, 49.9912), (10.0421, 49.9763), (10.0087, 49.9789)]]),           # across both blocks
    (302, [[(10.0031, 49.9741), (10.0243, 49.9737), (10.0239, 49.9623), (10.0027, 49.9629)],
           [(10.0091, 49.9712), (10.0093, 49.9661), (10.0187, 49.9657), (10.0183, 49.9709)]]),           # with a hole
    (303, [[(10.0313, 49.9733), (10.0497, 49.9741), (10.0489, 49.9627), (10.0307, 49.9633)]]),
    (304, [[(10.0411, 49.9691), (10.0557, 49.9687), (10.0553, 49.9611), (10.0407, 49.9617)]]),           # overlaps 303
    (305, [[(10.0567, 49.9951), (10.0581, 49.9949), (10.0579, 49.9903)]]),                               # outside every block
    (306, None),                                                                                         # a null shape
    (301, [[(10.0261, 49.9993), (10.0297, 49.9991), (10.0293, 49.9967), (10.0263, 49.9969)]]),           # a duplicate id
]


def _run(cwd, *args):
    return subprocess.run([GCN10, *args], cwd=str(cwd), capture_output=True, text=True, timeout=300)


def _oracle_blocks(esa, soil, tables):
    """per block: its window, clipped geotransform, box and the oracle's 18 rasters"""
    out = []
    for _bid, *bbox in BLOCKS:
        xo, yo, W, H, gt = oc.window(ESA_GT, RX, RY, bbox)
        sxo, syo, hsx, hsy, sgt = oc.window(SOIL_GT, soil.shape[1], soil.shape[0], bbox)
        cn = oc.process_block_mem(esa[yo:yo + H, xo:xo + W], gt, soil[syo:syo + hsy, sxo:sxo + hsx], sgt, tables)
        out.append((xo, yo, W, H, gt, bbox, cn))
    return out


def _expected(blocks, zones):
    """per zone record and raster: [pixels, valid, sum, sum of squares, min, max] in Python integers"""
    want = [[[0, 0, 0, 0, 255, 0] for _r in range(18)] for _z in zones]
    for _xo, _yo, W, H, gt, bbox, cn in blocks:
        own = zoneutil.own_mask(gt, W, H, bbox)
        for zi, (_id, rings) in enumerate(zones):
            if rings is None:
                continue
            mask = zoneutil.zone_mask(rings, gt, W, H) & own
            for r in range(18):
                v = cn[r][mask].astype(np.int64)
                ok = v[v != 255]
                c = want[zi][r]
                c[0] += int(v.size)
                c[1] += int(ok.size)
                c[2] += int(ok.sum())
                c[3] += int((ok * ok).sum())
                if ok.size:
                    c[4], c[5] = min(c[4], int(ok.min())), max(c[5], int(ok.max()))
    return want


@pytest.fixture(scope="module")
def world(tmp_path_factory, tables):
    d = tmp_path_factory.mktemp("zonal")
    rng = np.random.default_rng(11)
    small = rng.choice(ESA_NASTY, size=(RY // 20, RX // 20))
    esa = np.repeat(np.repeat(small, 20, axis=0), 20, axis=1)
    noise = rng.integers(0, 256, size=esa.shape, dtype=np.uint8)
    esa = np.where(noise < 40, rng.choice(ESA_NASTY, size=esa.shape), esa).astype(np.uint8)
    esa[300:380, 100:260] = 0               # landcover NoData inside zone 302: pixels that are not valid
    soil = rng.choice(HSG_NASTY, size=(28, 36)).astype(np.uint8)
    tiffutil.write_tiff(str(d / "esa.tif"), esa, gt=ESA_GT, compression=8, tile=(256, 256))
    tiffutil.write_tiff(str(d / "soil.tif"), soil, gt=SOIL_GT, compression=5, rows_per_strip=8)
    tiffutil.write_block_shapefile(str(d / "blocks"), BLOCKS)
    zoneutil.write_zone_shapefile(str(d / "zones"), ZONES)
    for n in (1, 2):
        (d / ("config%d.txt" % n)).write_text(
            "hysogs_data_path=%s\nesa_data_path=%s\nblocks_shp_path=%s\nlookup_table_path=%s\nlog_dir=%s\n"
            "io_threads=4\nworkers_per_gpu=%d\nzonal_output=table%d.csv\n"
            % (d / "soil.tif", d / "esa.tif", d / "blocks.shp", LOOKUPS, d / ("logs%d" % n), n, n))
    wins = [oc.window(ESA_GT, RX, RY, b[1:]) for b in BLOCKS]
    assert wins[0][0] + wins[0][2] == wins[1][0] + 1        # the blocks' windows share one pixel column
    out = _run(d, "-c", "config1.txt", "--zones", "zones.shp")
    blocks = _oracle_blocks(esa, soil, tables)
    return {"dir": d, "esa": esa, "soil": soil, "blocks": blocks, "want": _expected(blocks, ZONES), "run1": out}


def _rows(path):
    lines = open(path).read().split("\n")
    assert lines[0] == "zone_id,condition,hc,arc,pixels,valid,sum,mean,min,max,stddev" and lines[-1] == ""
    return [ln.split(",") for ln in lines[1:-1]]


def _check_rows(rows, want, sel, zones=ZONES):
    assert len(rows) == len(zones) * len(sel)
    it = iter(rows)
    for zi, (zid, _rings) in enumerate(zones):          # one row per zone record, file order, x selected raster
        for r in sel:
            row = next(it)
            pixels, valid, total, sq, lo, hi = want[zi][r]
            c, k = divmod(r, 9)
            assert row[:4] == [str(zid), CONDS[c], HCS[k // 3], ARCS[k % 3]]
            assert [int(x) for x in row[4:7]] == [pixels, valid, total], row
            if valid == 0:
                assert row[7:] == ["", "", "", ""], row
                continue
            assert row[7] == "%.14g" % (total / valid), row
            assert [int(row[8]), int(row[9])] == [lo, hi], row
            sd = math.sqrt(valid * sq - total * total) / valid
            assert abs(float(row[10]) - sd) <= 1e-12 * max(sd, 1e-300), (row, sd)


def test_the_table_equals_the_oracle_rasters_masked_by_the_zones(world):
    out, d, want = world["run1"], world["dir"], world["want"]
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    # the fixture means something: every kind of zone has the pixels it should
    assert want[0][0][0] > 20000 and want[4][0][0] == 0 and want[5][0][0] == 0 and want[6][0][0] > 0
    assert want[1][0][1] < want[1][0][0]                # zone 302 has pixels that are not valid
    _check_rows(_rows(d / "table1.csv"), want, range(18))
    assert "zonal: 2 blocks, 7 zones, 2 without pixels, table table1.csv" in out.stderr
    log = (d / "logs1" / "rank_0.log").read_text()
    assert "zonal block 7: " in log and "zonal block 8: " in log and " zones, " in log and " spans" in log
    assert not [f for f in os.listdir(d) if f.startswith("cn_rasters_") or ".part" in f]
    assert not (d / "zonal_cn.csv").exists()            # zonal_output names the table


def test_a_tessellation_across_both_blocks_counts_every_owned_pixel_of_its_hull_once(world):
    """A second zone file: a lattice of 8 x 7 cells of 80 x 60 px with every vertex on a pixel centre of the landcover
    grid, two triangles per cell, across the blocks' shared column 336.  Its diagonals pass through a centre every
    (4, 3) pixels.  The table against the oracle as above; and per raster the zones' pixels add up to the hull's, which a
    pixel on a shared edge counted by both neighbours or by neither would not."""
    d = world["dir"]
    rings, (x0, x1, y0, y1) = zoneutil.lattice_triangles(ESA_GT, 12, 8, 8, 7, 80, 60, seed=8)
    zones = [(500 + i, [r]) for i, r in enumerate(rings)]
    zoneutil.write_zone_shapefile(str(d / "lattice"), zones)
    cfg = (d / "config1.txt").read_text().replace("table1.csv", "table4.csv").replace("logs1", "logs4")
    (d / "config4.txt").write_text(cfg)
    out = _run(d, "-c", "config4.txt", "--zones", "lattice.shp")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    # the hull's owned pixels by the rule on every block's own centres; those equal the grid's at the hull's sides, so
    # that is the rectangle of the grid (a block's clipped geotransform can put a centre an ulp off the grid's)
    gpx, gpy = zoneutil.centres(ESA_GT, RX, RY)
    hull = 0
    for xo, yo, W, H, gt, bbox, _cn in world["blocks"]:
        bpx, bpy = zoneutil.centres(gt, W, H)
        assert all(bpx[c - xo] == gpx[c] for c in (x0, x1) if xo <= c < xo + W) and (bpy == gpy[yo:yo + H]).all()
        hull += int((zoneutil.hull_mask(gt, W, H, rings) & zoneutil.own_mask(gt, W, H, bbox)).sum())
    assert hull == (x1 - x0) * (y1 - y0) == 640 * 420 and x0 < 336 < x1
    want = _expected(world["blocks"], zones)
    assert min(w[0][0] for w in want) > 0               # every triangle has pixels
    rows = _rows(d / "table4.csv")
    _check_rows(rows, want, range(18), zones)
    for r in range(18):
        assert sum(int(row[4]) for row in rows[r::18]) == hull
    assert "zonal: 2 blocks, %d zones, 0 without pixels, table table4.csv" % len(zones) in out.stderr


def test_lookups_and_conditions_select_the_rows(world):
    d = world["dir"]
    out = _run(d, "-c", "config1.txt", "--zones", "zones.shp", "--lookups", "g_ii", "--conditions", "drained")
    assert out.returncode == 0, out.stderr[-2000:]
    _check_rows(_rows(d / "table1.csv"), world["want"], [7])
    assert not [f for f in os.listdir(d) if f.startswith("cn_rasters_")]


def test_two_workers_per_gpu_write_the_same_bytes(world):
    d = world["dir"]
    one = _run(d, "-c", "config1.txt", "--zones", "zones.shp")
    two = _run(d, "-c", "config2.txt", "--zonal", "--zones", "zones.shp")
    assert one.returncode == 0 and two.returncode == 0, one.stderr[-1000:] + two.stderr[-1000:]
    assert (d / "table2.csv").read_bytes() == (d / "table1.csv").read_bytes()
    assert not [f for f in os.listdir(d) if f.startswith("cn_rasters_")]


def test_an_unreadable_block_ends_with_exit_code_1_after_the_table(world, tmp_path):
    """A block id that the shapefile lacks: an ERROR line, the table of the other block, exit code 1."""
    d = world["dir"]
    (tmp_path / "ids.txt").write_text("7 99\n")
    cfg = (d / "config1.txt").read_text().replace("table1.csv", str(tmp_path / "t.csv")).replace("logs1", "logs3")
    (tmp_path / "config.txt").write_text(cfg)
    out = _run(tmp_path, "-c", "config.txt", "--zones", str(d / "zones.shp"), "-l", "ids.txt")
    assert out.returncode == 1, out.stderr[-2000:]
    assert "zonal block 99: its landcover or soil window could not be read" in out.stdout + out.stderr
    rows = _rows(tmp_path / "t.csv")
    assert len(rows) == len(ZONES) * 18 and "zonal: 1 blocks" in out.stderr
