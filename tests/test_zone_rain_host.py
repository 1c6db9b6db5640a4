"""CPU: the host side of the rainfall raster under zones (config keys zone_rain / zone_rain_unit): gcn10_zone_rain_cut
against a numpy model -- zoneutil.zone_mask times the cell maps of gcn10_grid_plan_block times the raster --, the sort
order, the items and both bounds; the refusals of gcn10_zone_rain_load on fixtures written with tests/tiffutil.py; the
closed forms of the table's columns (gcn10_zone_rain_values) on hand-worked triples; and the cutter as a stand-alone
program under AddressSanitizer + UBSan (tests/zone_rain_san_main.c)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from gcn10_amd import host
from tests import runoffutil as ru
from tests import tiffutil, zoneutil
from tests.conftest import ROOT

W, H = 203, 151
GT = zoneutil.TIE_GTS[0]
DX, DY = GT[1], -GT[5]


def at(u, v):
    """a point u, v pixels from the window's corner, off every pixel centre"""
    return (GT[0] + (u + 0.013) * DX, GT[3] - (v + 0.017) * DY)


# a zone with a hole, two zones that overlap, one that leaves the window, one of a few pixels
ZONES = [
    (11, [[at(10, 8), at(120, 12), at(110, 90), at(20, 100)], [at(40, 30), at(80, 32), at(78, 70), at(42, 66)]]),
    (12, [[at(90, 60), at(190, 50), at(180, 140), at(100, 130)]]),
    (13, [[at(150, 5), at(260, 20), at(230, 75), at(140, 80)]]),
    (14, [[at(5, 120), at(9, 121), at(8, 125), at(4, 124)]]),
]


def grid_of(cell_px, off=(0.3, 0.6), cover=(W, H), lead=2):
    """a raster of cell_px x cell_px pixel cells whose corner lies `lead` cells and a fraction outside the window"""
    dx, dy = cell_px * DX, cell_px * DY
    return {"xmin": GT[0] - (lead + off[0]) * dx, "ymax": GT[3] + (lead + off[1]) * dy, "dx": dx, "dy": dy,
            "nx": int(cover[0] / cell_px) + lead + 2, "ny": int(cover[1] / cell_px) + lead + 2}


def field_of(grid, seed, few=False):
    rng = np.random.default_rng(seed)
    if few:         # neighbours often share a byte: cells merge
        return rng.choice(np.array([0, 3, 3, 3, 200, 255], np.uint8), size=(grid["ny"], grid["nx"]))
    return rng.integers(0, 256, (grid["ny"], grid["nx"])).astype(np.uint8)


def rasters():
    fine, coarse = grid_of(7), grid_of(100)
    huge = {"xmin": GT[0] - 1.0, "ymax": GT[3] + 1.0, "dx": 100.0, "dy": 100.0, "nx": 1, "ny": 1}
    quarter = {"xmin": GT[0] - 3.3 * DX, "ymax": GT[3] + 2.2 * DY, "dx": 9 * DX, "dy": 11 * DY, "nx": 12, "ny": 7}
    return {
        "7 px cells": (fine, field_of(fine, 1)),
        "7 px cells, few bytes": (fine, field_of(fine, 2, few=True)),
        "100 px cells": (coarse, field_of(coarse, 3)),
        "one cell over the window": (huge, np.array([[77]], np.uint8)),
        "the north-west quarter": (quarter, field_of(quarter, 4)),
        "constant": (fine, np.full((fine["ny"], fine["nx"]), 20, np.uint8)),
    }


RASTERS = rasters()
BOUNDS = [(0, 0), (16, 16), (5, 64)]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    base = str(tmp_path_factory.mktemp("zr") / "z")
    zoneutil.write_zone_shapefile(base, ZONES)
    with host.Zones(base + ".shp") as z:
        p = z.build_plan(GT, W, H)
    assert p["local_zone"].tolist() == [0, 1, 2, 3]
    return p


def model(name):
    """(byte per pixel as int, -1 outside the raster; the cell maps' dict)"""
    grid, field = RASTERS[name]
    gp = host.grid_plan_block(grid, W, H, GT)
    byte = np.full((H, W), -1, np.int64)
    if gp["cellx"].size:
        cx, cy = gp["cellx"].astype(np.int64), gp["celly"].astype(np.int64)
        ys, xs = np.flatnonzero(cy >= 0), np.flatnonzero(cx >= 0)
        byte[np.ix_(ys, xs)] = field[(cy[ys] + gp["cy0"])[:, None], (cx[xs] + gp["cx0"])[None, :]]
    return byte, gp


def test_the_fixture_is_what_the_cases_say(plan):
    masks = [zoneutil.zone_mask(r, GT, W, H) for _id, r in ZONES]
    assert not masks[0][50, 60] and masks[0][20, 60]                # the hole
    assert (masks[0] & masks[1]).any()                              # the overlap
    assert masks[2][:, W - 1].any()                                 # cut by the window
    byte, _gp = model("the north-west quarter")
    assert (byte[:60, :90] >= 0).all() and (byte[80:, :] < 0).all() and (byte[:, 110:] < 0).all()
    byte, _gp = model("one cell over the window")
    assert (byte == 77).all()
    byte, gp = model("7 px cells")
    assert (byte >= 0).all() and gp["cx1"] - gp["cx0"] >= 29 and len(np.unique(byte)) > 200


@pytest.mark.parametrize("bounds", BOUNDS)
@pytest.mark.parametrize("name", sorted(RASTERS))
def test_cut_spans_equal_the_numpy_model(plan, name, bounds):
    byte, gp = model(name)
    cut = host.zone_rain_cut(plan, W, H, gp, RASTERS[name][1], *bounds)
    spans, items = cut["spans"], cut["items"]
    span_px, item_px = bounds
    # the table of every span, from its item; the items name every span once, in order, one zone and one byte each
    table = np.full(len(spans), -1, np.int64)
    at_span = 0
    for it in items:
        a, n = int(it["first_span"]), int(it["n_spans"])
        assert a == at_span and n > 0 and it["reserved"] == 0
        assert len(set(spans["zone"][a:a + n].tolist())) == 1
        table[a:a + n] = it["table"]
        if item_px:
            px = int((spans["x1"][a:a + n] - spans["x0"][a:a + n]).sum())
            assert px <= item_px or n == 1
        at_span += n
    assert at_span == len(spans)
    length = spans["x1"] - spans["x0"]
    assert (length > 0).all() and (length <= (span_px or 16384)).all()
    # sorted by (zone, byte, y, x0)
    keys = list(zip(spans["zone"].tolist(), table.tolist(), spans["y"].tolist(), spans["x0"].tolist()))
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    for li, (_id, rings) in enumerate(ZONES):
        mask = zoneutil.zone_mask(rings, GT, W, H)
        got = np.full((H, W), -1, np.int64)
        for s, t in zip(spans[spans["zone"] == li], table[spans["zone"] == li]):
            assert (got[s["y"], s["x0"]:s["x1"]] == -1).all(), "a pixel named twice"
            got[s["y"], s["x0"]:s["x1"]] = t
        want = np.where(mask, byte, -1)
        np.testing.assert_array_equal(got, want, err_msg="zone %d" % li)
        assert int(cut["rain_pixels"][li]) == int((want >= 0).sum())
        assert int(cut["rain_sum"][li]) == int(want[want >= 0].sum())


@pytest.mark.parametrize("name", sorted(RASTERS))
def test_the_bounds_change_no_pixel_and_no_item_key(plan, name):
    _byte, gp = model(name)
    cuts = [host.zone_rain_cut(plan, W, H, gp, RASTERS[name][1], *b) for b in BOUNDS]

    def pixels(cut):
        out = set()
        for it in cut["items"]:
            for s in cut["spans"][int(it["first_span"]):int(it["first_span"]) + int(it["n_spans"])]:
                out.update((int(s["zone"]), int(it["table"]), int(s["y"]), x) for x in range(s["x0"], s["x1"]))
        return out
    ref = pixels(cuts[0])
    for c in cuts[1:]:
        assert pixels(c) == ref
        np.testing.assert_array_equal(c["rain_pixels"], cuts[0]["rain_pixels"])
        np.testing.assert_array_equal(c["rain_sum"], cuts[0]["rain_sum"])
    assert len(cuts[1]["items"]) >= len(cuts[0]["items"]) and len(cuts[2]["spans"]) >= len(cuts[0]["spans"])


def test_a_constant_raster_gives_the_source_spans_merged(plan):
    """Under the default bounds the cut of a constant raster that covers everything is the plan itself."""
    _byte, gp = model("constant")
    cut = host.zone_rain_cut(plan, W, H, gp, RASTERS["constant"][1])
    np.testing.assert_array_equal(cut["spans"], plan["spans"])
    assert (cut["items"]["table"] == 20).all()
    np.testing.assert_array_equal(cut["rain_pixels"], plan["local_pixels"])
    np.testing.assert_array_equal(cut["rain_sum"], plan["local_pixels"] * 20)
    # ... and neighbouring cells of equal byte never cut a span
    _byte, gp = model("7 px cells, few bytes")
    few = host.zone_rain_cut(plan, W, H, gp, RASTERS["7 px cells, few bytes"][1])
    rnd = host.zone_rain_cut(plan, W, H, model("7 px cells")[1], RASTERS["7 px cells"][1])
    assert len(plan["spans"]) < len(few["spans"]) < len(rnd["spans"])


def test_a_block_outside_the_raster_has_no_span(plan):
    far = {"xmin": GT[0] + 500 * DX, "ymax": GT[3], "dx": DX * 10, "dy": DY * 10, "nx": 4, "ny": 4}
    gp = host.grid_plan_block(far, W, H, GT)
    cut = host.zone_rain_cut(plan, W, H, gp, np.full((4, 4), 9, np.uint8))
    assert len(cut["spans"]) == 0 and len(cut["items"]) == 0
    assert cut["rain_pixels"].tolist() == [0, 0, 0, 0] and cut["rain_sum"].tolist() == [0, 0, 0, 0]


def test_spans_outside_the_block_are_refused():
    gp = {"cellx": np.zeros(8, np.int32), "celly": np.zeros(4, np.int32), "cx0": 0, "cy0": 0}
    for bad in [(4, 0, 3, 0), (-1, 0, 3, 0), (1, 0, 9, 0), (1, -1, 3, 0), (1, 3, 3, 0), (1, 0, 3, 1), (1, 0, 3, -1)]:
        with pytest.raises(host.HostError):
            host.zone_rain_cut({"spans": np.array([bad], host.ZONE_SPAN_DTYPE)}, 8, 4, gp, np.zeros((1, 1), np.uint8),
                               n_local=1)


# ---- the loader ------------------------------------------------------------------------------------------------------

RGT = [10.0, 0.25, 0.0, 50.0, 0.0, -0.5]


def test_the_loader_returns_the_raster_as_a_grid(tmp_path):
    f = np.random.default_rng(1).integers(0, 256, (22, 30)).astype(np.uint8)
    path = str(tmp_path / "atlas.tif")
    tiffutil.write_tiff(path, f, gt=RGT, compression=8, tile=(16, 16))
    grid, got = host.zone_rain_load(path)
    assert grid == {"xmin": 10.0, "ymax": 50.0, "dx": 0.25, "dy": 0.5, "nx": 30, "ny": 22}
    np.testing.assert_array_equal(got, f)


def test_the_loader_refuses(tmp_path):
    def refusal(path):
        with pytest.raises(host.HostError) as e:
            host.zone_rain_load(path)
        return str(e.value)
    f = np.zeros((4, 6), np.uint8)
    none = str(tmp_path / "none.tif")
    assert refusal(none).startswith("zone_rain: cannot read '%s': " % none)
    (tmp_path / "text.tif").write_text("no tiff at all, but long enough to hold a header\n" * 4)
    assert refusal(str(tmp_path / "text.tif")).startswith("zone_rain: cannot read '%s': " % (tmp_path / "text.tif"))
    plain = str(tmp_path / "plain.tif")
    tiffutil.write_tiff(plain, f)
    assert refusal(plain) == "zone_rain: '%s' carries no geotransform" % plain
    for k, v in ((5, 0.5), (1, -0.25)):
        gt = list(RGT)
        gt[k] = v
        path = str(tmp_path / ("flip%d.tif" % k))
        tiffutil.write_tiff(path, f, gt=gt)
        assert refusal(path) == "zone_rain: '%s' is rotated or not north up" % path
    big = str(tmp_path / "big.tif")
    tiffutil.write_tiff(big, np.zeros((8193, 8192), np.uint8), gt=RGT, compression=8)
    assert refusal(big) == "zone_rain: '%s' has more than %d pixels" % (big, 1 << 26)


# ---- the columns -----------------------------------------------------------------------------------------------------

def test_the_columns_on_hand_worked_triples():
    v = host.zone_rain_values
    assert v(0, 0, 2.5, 0.2, 0, 0, 0) == (None, None, None)                 # no pixel in a rain cell
    assert v(10, 200, 2.5, 0.2, 0, 0, 0) == (50.0, None, None)              # rain, but no valid pixel
    # rain_mm == 0: the table is all zero, the rule gives the mean byte (round half up)
    assert v(4, 0, 2.5, 0.2, 301, 4, 0) == (0.0, 0.0, 75)
    assert v(4, 0, 2.5, 0.2, 302, 4, 0) == (0.0, 0.0, 76)
    # a constant field: rain_mm == b * unit bit for bit, and the columns of that storm
    for b, unit in ((20, 2.5), (7, 0.1), (255, 650.0 / 255.0), (3, 1.0 / 3.0)):
        for pixels in (1, 7, 70720, 3 * 10 ** 9):
            mm, _ro, _cn = v(pixels, pixels * b, unit, 0.2, 0, 0, 0)
            assert mm == b * unit and mm.hex() == (float(b) * unit).hex()
    q = ru.table(50.0, 0.2)
    values = np.array([60, 60, 80, 98], np.int64)
    s, n, sw = int(values.sum()), 4, int(q[values].astype(np.int64).sum())
    mm, ro, cn = v(4, 80, 2.5, 0.2, s, n, sw)
    assert mm == 50.0 and ro == sw / 4 / 100.0 and cn == ru.cn(s, n, sw, q) == host.runoff_cn(s, n, sw, q)
    assert cn > (2 * s + n) // (2 * n)                                      # Q is convex: above the mean CN
    # a field: the table is that of the MEAN depth, not of any cell's
    rain_sum, pixels = 3 * 10 + 1 * 40, 4
    mean_mm = (rain_sum / pixels) * 2.5
    t = host.runoff_table(mean_mm, 0.05)
    mm, ro, cn = v(pixels, rain_sum, 2.5, 0.05, s, n, 1234)
    assert mm == mean_mm and ro == 1234 / 4 / 100.0 and cn == host.runoff_cn(s, n, 1234, t)


# ---- the cutter under AddressSanitizer + UBSan -----------------------------------------------------------------------

def test_sanitized_program_cuts_every_case_and_truncation(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    exe = str(tmp_path / "zone_rain_san")
    cmd = [cc, "-std=c99", "-D_GNU_SOURCE", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-static-libasan", "-static-libubsan",
           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
           "-o", exe, os.path.join(ROOT, "tests", "zone_rain_san_main.c"),
           os.path.join(ROOT, "gcn10_amd", "csrc", "host", "zones.c"), "-lm"]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert "cases ok" in p.stdout
