"""CPU: the host side of several rainfall rasters under zones (config key zone_rains): gcn10_zone_rains_cut against a
numpy model -- zoneutil.zone_mask times the cell maps of gcn10_grid_plan_block times the k rasters --, the sort order by
(zone, tuple, y, x0), the items and both bounds, k identical layers against the one-layer cut; the two refusals that
gcn10_zone_rains_load adds and what it leaves allocated; the rule that forms the columns of zonal_cn.csv, for K = 1 and for each
layer of K > 1; and the cutter as a stand-alone program under AddressSanitizer + UBSan
(tests/zone_rains_san_main.c).  The window, the zones and the grids are those of tests/test_zone_rain_host.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from gcn10_amd import host
from tests import tiffutil, zoneutil
from tests.conftest import ROOT
from tests.test_zone_rain_host import BOUNDS, GT, H, W, ZONES, field_of, grid_of

KS = [1, 2, 3, 8]


def layers_of(grid, k, seed, kind):
    """k rasters on one grid: random bytes; few bytes, where the layers before the last are mostly equal, so that
    neighbouring cells share a tuple or differ in the last layer only; or one byte per layer"""
    rng = np.random.default_rng(seed)
    shape = (k, grid["ny"], grid["nx"])
    if kind == "random":
        return rng.integers(0, 256, shape).astype(np.uint8)
    if kind == "few":
        out = (rng.integers(0, 8, shape) == 0).astype(np.uint8) * 200
        out[k - 1] = rng.choice(np.array([0, 3, 3, 255], np.uint8), size=shape[1:])
        return out
    return np.broadcast_to((20 + np.arange(k, dtype=np.uint8))[:, None, None], shape).copy()


def grids():
    huge = {"xmin": GT[0] - 1.0, "ymax": GT[3] + 1.0, "dx": 100.0, "dy": 100.0, "nx": 1, "ny": 1}
    quarter = {"xmin": GT[0] - 3.3 * GT[1], "ymax": GT[3] - 2.2 * GT[5], "dx": 9 * GT[1], "dy": -11 * GT[5], "nx": 12,
               "ny": 7}
    return {"7 px cells": grid_of(7), "16 px cells": grid_of(16), "100 px cells": grid_of(100),
            "1000 px cells": grid_of(1000), "one cell over the window": huge, "the north-west quarter": quarter}


GRIDS = grids()
# (grid, kind of layers): every cell size with random layers, the small cells with few bytes and with one byte as well
CASES = [(g, "random") for g in sorted(GRIDS)] + [("7 px cells", "few"), ("16 px cells", "few"), ("7 px cells", "constant")]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    base = str(tmp_path_factory.mktemp("zrs") / "z")
    zoneutil.write_zone_shapefile(base, ZONES)
    with host.Zones(base + ".shp") as z:
        p = z.build_plan(GT, W, H)
    assert p["local_zone"].tolist() == [0, 1, 2, 3]
    return p


def model(grid, layers):
    """(the bytes of every pixel, int64[k][H][W], -1 outside the rasters; the cell maps' dict)"""
    gp = host.grid_plan_block(grid, W, H, GT)
    byte = np.full((len(layers), H, W), -1, np.int64)
    if gp["cellx"].size:
        cx, cy = gp["cellx"].astype(np.int64), gp["celly"].astype(np.int64)
        ys, xs = np.flatnonzero(cy >= 0), np.flatnonzero(cx >= 0)
        for j, field in enumerate(layers):
            byte[j][np.ix_(ys, xs)] = field[(cy[ys] + gp["cy0"])[:, None], (cx[xs] + gp["cx0"])[None, :]]
    return byte, gp


def test_the_fixture_is_what_the_cases_say():
    byte, gp = model(GRIDS["the north-west quarter"], layers_of(GRIDS["the north-west quarter"], 2, 1, "random"))
    assert (byte[:, :60, :90] >= 0).all() and (byte[:, 80:, :] < 0).all() and (byte[:, :, 110:] < 0).all()  # truncated maps
    assert (gp["cellx"] < 0).any() and (gp["celly"] < 0).any()
    few = layers_of(GRIDS["7 px cells"], 3, 2, "few")
    same_but_last = (few[:2, :, 1:] == few[:2, :, :-1]).all(axis=0) & (few[2, :, 1:] != few[2, :, :-1])
    assert same_but_last.any()                          # neighbours that differ in the last layer only
    assert (few[:, :, 1:] == few[:, :, :-1]).all(axis=0).any()      # ... and neighbours of equal tuple


@pytest.mark.parametrize("bounds", BOUNDS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s, %s" % c)
def test_cut_spans_equal_the_numpy_model(plan, case, k, bounds):
    grid = GRIDS[case[0]]
    layers = layers_of(grid, k, 10 * k + len(case[0]), case[1])
    byte, gp = model(grid, layers)
    cut = host.zone_rains_cut(plan, W, H, gp, layers, *bounds)
    spans, items = cut["spans"], cut["items"]
    span_px, item_px = bounds
    assert items["table"].shape == (len(items), 8) and (items["table"][:, k:] == 0).all()     # bytes K..7 are zero
    # the tuple of every span, from its item; the items name every span once, in order, one zone and one tuple each
    table = np.full((len(spans), 8), -1, np.int64)
    at_span = 0
    for it in items:
        a, n = int(it["first_span"]), int(it["n_spans"])
        assert a == at_span and n > 0
        assert len(set(spans["zone"][a:a + n].tolist())) == 1
        table[a:a + n] = it["table"]
        if item_px:
            px = int((spans["x1"][a:a + n] - spans["x0"][a:a + n]).sum())
            assert px <= item_px or n == 1
        at_span += n
    assert at_span == len(spans)
    length = spans["x1"] - spans["x0"]
    assert (length > 0).all() and (length <= (span_px or 16384)).all()
    # sorted by (zone, tuple, y, x0), the tuples in lexicographic order
    keys = [(z, tuple(t), y, x) for z, t, y, x in zip(spans["zone"].tolist(), table.tolist(), spans["y"].tolist(),
                                                      spans["x0"].tolist())]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert cut["rain_sum"].shape == (k, 4)
    for li, (_id, rings) in enumerate(ZONES):
        mask = zoneutil.zone_mask(rings, GT, W, H)
        got = np.full((k, H, W), -1, np.int64)
        for s, t in zip(spans[spans["zone"] == li], table[spans["zone"] == li]):
            assert (got[0, s["y"], s["x0"]:s["x1"]] == -1).all(), "a pixel named twice"
            got[:, s["y"], s["x0"]:s["x1"]] = t[:k, None]
        want = np.where(mask[None], byte, -1)
        np.testing.assert_array_equal(got, want, err_msg="zone %d" % li)       # every source pixel in the raster, once
        assert int(cut["rain_pixels"][li]) == int((want[0] >= 0).sum())
        for j in range(k):
            assert int(cut["rain_sum"][j][li]) == int(want[j][want[j] >= 0].sum())


@pytest.mark.parametrize("k", KS)
def test_the_bounds_change_no_pixel_and_no_item_key(plan, k):
    grid = GRIDS["7 px cells"]
    layers = layers_of(grid, k, 77 + k, "few")
    _byte, gp = model(grid, layers)
    cuts = [host.zone_rains_cut(plan, W, H, gp, layers, *b) for b in BOUNDS]

    def pixels(cut):
        out = set()
        for it in cut["items"]:
            for s in cut["spans"][int(it["first_span"]):int(it["first_span"]) + int(it["n_spans"])]:
                out.update((int(s["zone"]), bytes(it["table"]), int(s["y"]), x) for x in range(s["x0"], s["x1"]))
        return out
    ref = pixels(cuts[0])
    for c in cuts[1:]:
        assert pixels(c) == ref
        np.testing.assert_array_equal(c["rain_pixels"], cuts[0]["rain_pixels"])
        np.testing.assert_array_equal(c["rain_sum"], cuts[0]["rain_sum"])
    assert len(cuts[1]["items"]) >= len(cuts[0]["items"]) and len(cuts[2]["spans"]) >= len(cuts[0]["spans"])


@pytest.mark.parametrize("bounds", BOUNDS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["7 px cells", "100 px cells", "the north-west quarter"])
def test_identical_layers_are_the_one_layer_cut_with_the_byte_repeated(plan, name, k, bounds):
    grid = GRIDS[name]
    field = field_of(grid, 5, few=name == "7 px cells")
    gp = host.grid_plan_block(grid, W, H, GT)
    one = host.zone_rain_cut(plan, W, H, gp, field, *bounds)
    many = host.zone_rains_cut(plan, W, H, gp, np.stack([field] * k), *bounds)
    np.testing.assert_array_equal(many["spans"], one["spans"])
    np.testing.assert_array_equal(many["items"]["first_span"], one["items"]["first_span"])
    np.testing.assert_array_equal(many["items"]["n_spans"], one["items"]["n_spans"])
    want = np.zeros((len(one["items"]), 8), np.uint8)
    want[:, :k] = one["items"]["table"][:, None]
    np.testing.assert_array_equal(many["items"]["table"], want)
    np.testing.assert_array_equal(many["rain_pixels"], one["rain_pixels"])
    for j in range(k):
        np.testing.assert_array_equal(many["rain_sum"][j], one["rain_sum"])


def test_a_layer_that_differs_somewhere_cuts_there_and_nowhere_else(plan):
    """One cell of the last layer differs: the cut has more spans than the one-layer cut, and only pixels of that cell
    come under another tuple."""
    grid = GRIDS["16 px cells"]
    base = np.full((grid["ny"], grid["nx"]), 9, np.uint8)
    other = base.copy()
    other[3, 5] = 10
    gp = host.grid_plan_block(grid, W, H, GT)
    same = host.zone_rains_cut(plan, W, H, gp, np.stack([base, base, base]))
    cut = host.zone_rains_cut(plan, W, H, gp, np.stack([base, base, other]))
    assert len(cut["spans"]) > len(same["spans"]) == len(plan["spans"])
    tuples = sorted(set(bytes(t) for t in cut["items"]["table"]))
    assert tuples == [bytes([9, 9, 9, 0, 0, 0, 0, 0]), bytes([9, 9, 10, 0, 0, 0, 0, 0])]
    np.testing.assert_array_equal(cut["rain_pixels"], same["rain_pixels"])
    np.testing.assert_array_equal(cut["rain_sum"][:2], same["rain_sum"][:2])
    px = int((gp["cellx"] + gp["cx0"] == 5).sum()) * int((gp["celly"] + gp["cy0"] == 3).sum())
    assert 0 < int((cut["rain_sum"][2] - same["rain_sum"][2]).sum()) <= px * len(ZONES)


def test_a_block_outside_the_rasters_and_bad_arguments(plan):
    far = {"xmin": GT[0] + 500 * GT[1], "ymax": GT[3], "dx": GT[1] * 10, "dy": -GT[5] * 10, "nx": 4, "ny": 4}
    gp = host.grid_plan_block(far, W, H, GT)
    cut = host.zone_rains_cut(plan, W, H, gp, np.full((2, 4, 4), 9, np.uint8))
    assert len(cut["spans"]) == 0 and len(cut["items"]) == 0
    assert cut["rain_pixels"].tolist() == [0, 0, 0, 0] and cut["rain_sum"].tolist() == [[0, 0, 0, 0]] * 2
    near = host.grid_plan_block(GRIDS["100 px cells"], W, H, GT)
    for k in (0, 9):
        with pytest.raises((host.HostError, ValueError)):
            host.zone_rains_cut(plan, W, H, near, np.zeros((k, GRIDS["100 px cells"]["ny"], GRIDS["100 px cells"]["nx"]),
                                                           np.uint8))
    gp = {"cellx": np.zeros(8, np.int32), "celly": np.zeros(4, np.int32), "cx0": 0, "cy0": 0}
    for bad in [(4, 0, 3, 0), (-1, 0, 3, 0), (1, 0, 9, 0), (1, -1, 3, 0), (1, 3, 3, 0), (1, 0, 3, 1), (1, 0, 3, -1)]:
        with pytest.raises(host.HostError):
            host.zone_rains_cut({"spans": np.array([bad], host.ZONE_SPAN_DTYPE)}, 8, 4, gp, np.zeros((2, 1, 1), np.uint8),
                                n_local=1)


# ---- the loader ------------------------------------------------------------------------------------------------------

RGT = [10.0, 0.25, 0.0, 50.0, 0.0, -0.5]


def _write(path, shape=(22, 30), gt=RGT, seed=1, **kw):
    f = np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)
    tiffutil.write_tiff(str(path), f, gt=gt, **kw)
    return f


def test_the_loader_returns_the_rasters_on_the_grid_of_the_first(tmp_path):
    fields = [_write(tmp_path / ("r%d.tif" % j), seed=j, compression=8 if j else 1) for j in range(3)]
    grid, got = host.zone_rains_load([str(tmp_path / ("r%d.tif" % j)) for j in range(3)])
    assert grid == {"xmin": 10.0, "ymax": 50.0, "dx": 0.25, "dy": 0.5, "nx": 30, "ny": 22}
    np.testing.assert_array_equal(got, np.stack(fields))
    grid, got = host.zone_rains_load([str(tmp_path / "r2.tif")])
    assert got.shape == (1, 22, 30) and (got[0] == fields[2]).all()


def test_the_loader_refuses_and_leaves_nothing_allocated(tmp_path):
    def refusal(*paths):
        with pytest.raises(host.HostError) as e:
            host.zone_rains_load([str(p) for p in paths])
        assert e.value.left == [None] * 8           # nothing stays allocated: every layer read so far was freed
        return str(e.value)
    first = tmp_path / "first.tif"
    _write(first)
    # every rule of zone_rain, under the prefix of this key, for the first file and for a later one
    none = tmp_path / "none.tif"
    assert refusal(none).startswith("zone_rains: cannot read '%s': " % none)
    assert refusal(first, first, none).startswith("zone_rains: cannot read '%s': " % none)
    plain = tmp_path / "plain.tif"
    tiffutil.write_tiff(str(plain), np.zeros((22, 30), np.uint8))
    assert refusal(first, plain) == "zone_rains: '%s' carries no geotransform" % plain
    flip = tmp_path / "flip.tif"
    _write(flip, gt=[10.0, 0.25, 0.0, 50.0, 0.0, 0.5])
    assert refusal(flip, first) == refusal(first, flip) == "zone_rains: '%s' is rotated or not north up" % flip
    # another size than the first file's
    for shape in ((22, 31), (21, 30), (30, 22)):
        other = tmp_path / ("size_%d_%d.tif" % shape)
        _write(other, shape=shape)
        assert refusal(first, first, other) == ("zone_rains: '%s' has %d x %d pixels, '%s' has 30 x 22"
                                                % (other, shape[1], shape[0], first))
    # another geotransform: one double off by one unit in the last place, each of the four in turn
    for i in (0, 1, 3, 5):
        gt = list(RGT)
        gt[i] = float(np.nextafter(gt[i], 1e9))
        off = tmp_path / ("off%d.tif" % i)
        _write(off, gt=gt)
        assert refusal(first, off) == ("zone_rains: '%s' does not lie on the grid of '%s' (origin %.17g, %.17g, pixel "
                                       "%.17g x %.17g)" % (off, first, gt[0], gt[3], gt[1], gt[5]))
    # the size is looked at before the geotransform, the files in the order given
    assert "has 31 x 22 pixels" in refusal(first, tmp_path / "size_22_31.tif", tmp_path / "off0.tif")
    assert "does not lie on the grid" in refusal(first, tmp_path / "off0.tif", tmp_path / "size_22_31.tif")


# ---- the columns of the table ----------------------------------------------------------------------------------------

def test_each_triple_is_formed_by_the_values_rule_of_one_raster():
    """gcn10_zone_rain_values(rain_pixels, rain_sum_j, unit, lambda, s, n, sw_j): layer j's three fields depend on
    rain_sum_j and sw_j only, so they are what the one-raster run prints -- empty fields included."""
    v = host.zone_rain_values
    s, n, pixels = 301, 4, 6
    sums, sws = [0, 60, 1530], [0, 1234, 99999]
    triples = [v(pixels, sums[j], 2.5, 0.2, s, n, sws[j]) for j in range(3)]
    assert triples[0] == (0.0, 0.0, 75)                         # no rain: the mean byte
    assert triples[1][0] == 25.0 and triples[1][1] == 1234 / 4 / 100.0
    assert triples[2][0] == 637.5 and triples[2][2] == host.runoff_cn(s, n, 99999, host.runoff_table(637.5, 0.2))
    assert v(pixels, 60, 2.5, 0.2, 0, 0, 0) == (25.0, None, None)       # rain, no valid pixel: two empty fields
    assert v(0, 0, 2.5, 0.2, 0, 0, 0) == (None, None, None)             # no pixel in a cell: three


# ---- the cutter under AddressSanitizer + UBSan -----------------------------------------------------------------------

def test_sanitized_program_cuts_every_case_and_truncation(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    exe = str(tmp_path / "zone_rains_san")
    cmd = [cc, "-std=c99", "-D_GNU_SOURCE", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-static-libasan", "-static-libubsan",
           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
           "-o", exe, os.path.join(ROOT, "tests", "zone_rains_san_main.c"),
           os.path.join(ROOT, "gcn10_amd", "csrc", "host", "zones.c"), "-lm"]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert "cases ok" in p.stdout
