"""GPU: a landcover tile whose DEFLATE stream does not decode, in every kind of run.  The decoder answers such a stream
with a status word, which the worker reads when it takes the staged block over.  tests/test_cli.py holds the write run
to that; here the small world of that file (3000 px of landcover, blocks 101 and 102, the damaged tile read by block 102
only) goes through --verify, --zones, --grid and --aggregate: the same two lines about the window, each kind of run's
own answer to a block it cannot read, and block 101's result as it comes out of a run that has block 101 alone and an
undamaged landcover."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

from tests import zoneutil
from tests.conftest import ROOT
from tests.test_cli import _world

pytestmark = pytest.mark.gpu

GCN10 = os.path.join(ROOT, "bin", "gcn10")
CONDS, HCS, ARCS = ("drained", "undrained"), ("p", "f", "g"), ("i", "ii", "iii")
ZONES = [
    (401, [[(10.2, 49.8), (10.6, 49.8), (10.6, 49.3), (10.2, 49.3)]]),         # inside block 101
    (402, [[(11.3, 48.7), (11.7, 48.7), (11.7, 48.2), (11.3, 48.2)]]),         # inside block 102
    (403, [[(10.8, 49.2), (11.2, 49.2), (11.2, 48.8), (10.8, 48.8)]]),         # over the corner the two blocks share
]
GRID_TEXT = "10,50,0.05,0.05,40,40"         # cells of 50 px over both blocks
KINDS = {"zones": ("--zones", "zones.shp"), "grid": ("--grid", GRID_TEXT), "aggregate": ("--aggregate", "25")}


def _dir(d, name):
    """a run directory of its own (the outputs go to the working directory), with its config and log directory"""
    (d / name).mkdir()
    cfg = (d / "config.txt").read_text()
    assert "log_dir=%s\n" % (d / "logs") in cfg
    (d / name / "config.txt").write_text(cfg.replace("log_dir=%s\n" % (d / "logs"), "log_dir=%s\n" % (d / name / "logs")))
    return d / name


def _run(d, name, ids, *args):
    args = [str(d / a) if a == "zones.shp" else a for a in args]
    out = subprocess.run([GCN10, "-c", "config.txt", "-l", str(d / ids), *args], cwd=str(d / name), capture_output=True,
                         text=True, timeout=300)
    logs = d / name / "logs"
    log = "".join((logs / f).read_text() for f in sorted(os.listdir(logs)) if f.endswith(".log"))
    return out, out.stdout + out.stderr + log


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    d = tmp_path_factory.mktemp("unreadable")
    _world(d, seed=78)
    zoneutil.write_zone_shapefile(str(d / "zones"), ZONES)
    (d / "both.txt").write_text("101 102\n")
    (d / "alone.txt").write_text("101\n")
    # before the damage: the rasters that the verify run reads, and block 101 alone in the other kinds of run
    _dir(d, "verify")
    out, text = _run(d, "verify", "both.txt")
    assert out.returncode == 0, text[-2000:]
    shutil.rmtree(d / "verify" / "logs")                # the logs append: the verify run starts its own
    for kind, args in KINDS.items():
        _dir(d, kind + "_alone")
        out, text = _run(d, kind + "_alone", "alone.txt", *args)
        assert out.returncode == 0 and "ERROR" not in text, text[-2000:]
    # the damage of tests/test_cli.py's test_corrupt_landcover_tile_fails_its_block_only
    path = d / "esa.tif"
    raw = bytearray(path.read_bytes())
    im = Image.open(str(path))
    offs, cnts = im.tag_v2[324], im.tag_v2[325]
    across = (3000 + 511) // 512
    k = 2 * across + 3                                  # tile (row 2, col 3): rows 1024.., columns 1536..: block 102 only
    for i in range(offs[k] + 2, offs[k] + cnts[k]):
        raw[i] = 0xFF
    path.write_bytes(bytes(raw))
    return d


def _shared_lines(text):
    assert "gdalrasterio error: cannot decode a tile of the window" in text
    assert "esa load failed for block 102" in text
    assert "esa load failed for block 101" not in text


def _rasters(run, pattern):
    out = []
    for r in range(18):
        c, k = divmod(r, 9)
        with Image.open(str(run / (pattern % (CONDS[c], HCS[k // 3], ARCS[k % 3])))) as im:
            out.append(np.array(im))
    return out


def test_verify_counts_the_block_as_unreadable_and_verifies_its_neighbour(world):
    d = world
    out, text = _run(d, "verify", "both.txt", "--verify")
    assert out.returncode == 2, text[-2000:]
    _shared_lines(text)
    assert "UNREADABLE block 102: its landcover or soil window could not be read, 18 rasters not verified" in text
    assert (d / "verify" / "logs" / "verify_failed_blocks.txt").read_text() == "102\n"
    assert text.count("verified block 101: ") == 18
    assert "verify: 2 blocks, 18 files verified, 18 bad, 0 missing, 0 overview levels not checked" in text


def test_zones_write_the_table_without_the_block_and_end_with_1(world):
    d = world
    _dir(d, "zones_both")
    out, text = _run(d, "zones_both", "both.txt", *KINDS["zones"])
    assert out.returncode == 1, text[-2000:]
    _shared_lines(text)
    assert ("zonal block 102: its landcover or soil window could not be read; the table lacks this block") in text
    assert "zonal: 1 blocks, 3 zones, 1 without pixels, table zonal_cn.csv" in text
    table = (d / "zones_both" / "zonal_cn.csv").read_text()
    assert table == (d / "zones_alone" / "zonal_cn.csv").read_text()
    rows = [ln.split(",") for ln in table.split("\n")[1:-1]]
    assert len(rows) == 3 * 18
    assert int(rows[0][4]) > 100000 and int(rows[18][4]) == 0 and int(rows[36][4]) > 10000      # 401, 402, 403: pixels


def test_grid_writes_the_rasters_without_the_block_and_ends_with_1(world):
    d = world
    _dir(d, "grid_both")
    out, text = _run(d, "grid_both", "both.txt", *KINDS["grid"])
    assert out.returncode == 1, text[-2000:]
    _shared_lines(text)
    assert "grid block 102: its landcover or soil window could not be read; the rasters lack this block" in text
    assert "grid: 1 blocks, 18 rasters of 40 x 40 cells" in text
    got, want = _rasters(d / "grid_both", "cn_grid_%s/cn_%s_%s.tif"), _rasters(d / "grid_alone", "cn_grid_%s/cn_%s_%s.tif")
    for r in range(18):
        assert got[r].shape == (40, 40) and np.array_equal(got[r], want[r]), r
        assert (got[r][:20, :20] != 255).any() and (got[r][20:, 20:] == 255).all(), r       # block 101's cells, 102's
    for c in CONDS:
        assert not [f for f in os.listdir(d / "grid_both" / ("cn_grid_%s" % c)) if ".part" in f]


def test_aggregate_skips_the_block_leaves_no_file_of_it_and_ends_with_0(world):
    d = world
    _dir(d, "aggregate_both")
    out, text = _run(d, "aggregate_both", "both.txt", *KINDS["aggregate"])
    assert out.returncode == 0, text[-2000:]
    _shared_lines(text)
    for c in CONDS:
        names = sorted(os.listdir(d / "aggregate_both" / ("cn_rasters_%s_x25" % c)))
        assert names == sorted("cn_%s_%s_101.tif" % (hc, arc) for hc in HCS for arc in ARCS), names     # no _102, no .part
    got = _rasters(d / "aggregate_both", "cn_rasters_%s_x25/cn_%s_%s_101.tif")
    want = _rasters(d / "aggregate_alone", "cn_rasters_%s_x25/cn_%s_%s_101.tif")
    for r in range(18):
        assert got[r].shape == (40, 40) and np.array_equal(got[r], want[r]), r
    assert text.count("completed condition for 101: ") == 18 and "completed condition for 102: " not in text
