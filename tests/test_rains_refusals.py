"""CPU: every way a run with several rainfall rasters (config key rains, --rains) stops before a GPU is opened: exit
status 1, the exact text on stderr, nothing created -- run the way tests/test_rain_refusals.py runs its table, with its
rasters --; the order in which the refusals are tested; that rain_unit alone still asks for rain; then the start-up
failure on a GPU library that lacks the entry points (the stub of tests/stub_gpu), and that a run with rain alone asks
for the _rain calls as before."""
import pytest

from tests.test_grid_refusals import GRID, _config, _gcn10, _nothing_written, stub, zones  # noqa: F401
from tests.test_rain_refusals import _bad, rain  # noqa: F401  (the unit's message, and the four rasters)


def _bad_rains(text):
    return "[rank 0] bad value for rains: '%s' (file1[:file2...]: 1 to 8 files)\n" % text


R = "{d}/rain.tif:{d}/plain.tif"
NINE = ":".join(["{d}/rain.tif"] * 9)

# name -> (config keys, arguments behind "-c <config>", stderr); "{zones}" stands for the zone file, "{d}" for the folder
# of the rasters
REFUSALS = {
    "rain_unit alone": ({}, ["--rain-unit", "2", "--grid", GRID], "[rank 0] rain_unit needs rain\n"),
    "rain_unit key alone": (dict(rain_unit="2,0.1", grid=GRID), [], "[rank 0] rain_unit needs rain\n"),
    "rains with --rain": ({}, ["--rains", R, "--rain", "{d}/rain.tif", "--grid", GRID],
                          "[rank 0] rains cannot be combined with rain\n"),
    "rains key with the rain key": (dict(rains=R, rain="{d}/rain.tif", grid=GRID), [],
                                    "[rank 0] rains cannot be combined with rain\n"),
    "rains with the rain key": (dict(rain="{d}/rain.tif", grid=GRID), ["--rains", R],
                                "[rank 0] rains cannot be combined with rain\n"),
    "rains alone": ({}, ["--rains", R], "[rank 0] rains needs --grid\n"),
    "rains key alone": (dict(rains=R, rain_unit="2"), [], "[rank 0] rains needs --grid\n"),
    "rains with --storm": ({}, ["--rains", R, "--grid", GRID, "--storm", "50"],
                           "[rank 0] rains cannot be combined with storm\n"),
    "rains key with the storm key": (dict(rains=R, grid=GRID, storm="50"), [],
                                     "[rank 0] rains cannot be combined with storm\n"),
    "rains with --storms": ({}, ["--rains", R, "--grid", GRID, "--storms", "25:50"],
                            "[rank 0] rains cannot be combined with storms\n"),
    "rains with the storms key": (dict(storms="25:50", grid=GRID), ["--rains", R],
                                  "[rank 0] rains cannot be combined with storms\n"),
    "rains with --verify": ({}, ["--rains", R, "--grid", GRID, "--verify"],
                            "[rank 0] rains cannot be combined with --verify\n"),
    "rains with --aggregate": ({}, ["--rains", R, "--grid", GRID, "--aggregate", "25"],
                               "[rank 0] rains cannot be combined with aggregate\n"),
    "rains key with aggregate=7": (dict(rains=R, aggregate=7), [], "[rank 0] rains cannot be combined with aggregate\n"),
    "rains with --zonal": ({}, ["--rains", R, "--zones", "{zones}"], "[rank 0] rains cannot be combined with --zonal\n"),
    "rains key with zonal=1": (dict(rains=R, zonal=1, zones_shp_path="{zones}", grid=GRID), [],
                               "[rank 0] rains cannot be combined with --zonal\n"),
    # the order: rain, verify, aggregate, zonal, storm / storms, no grid, the value, the unit, the files
    "order: rain first": ({}, ["--rains", R, "--rain", "{d}/rain.tif", "--verify", "--aggregate", "25", "--storm", "50"],
                          "[rank 0] rains cannot be combined with rain\n"),
    "order: verify before aggregate": ({}, ["--rains", R, "--verify", "--aggregate", "25", "--zones", "{zones}",
                                            "--storm", "50"], "[rank 0] rains cannot be combined with --verify\n"),
    "order: aggregate before zonal": ({}, ["--rains", R, "--aggregate", "25", "--zones", "{zones}"],
                                      "[rank 0] rains cannot be combined with aggregate\n"),
    "order: zonal before storm": ({}, ["--rains", R, "--zones", "{zones}", "--storm", "50"],
                                  "[rank 0] rains cannot be combined with --zonal\n"),
    "order: storm before no grid": ({}, ["--rains", R, "--storm", "50"], "[rank 0] rains cannot be combined with storm\n"),
    "order: storms before no grid": ({}, ["--rains", R, "--storms", "25:50"],
                                     "[rank 0] rains cannot be combined with storms\n"),
    "order: no grid before a bad value": ({}, ["--rains", ":"], "[rank 0] rains needs --grid\n"),
    "order: a bad value before a bad unit": ({}, ["--rains", "{d}/rain.tif:", "--rain-unit", "x", "--grid", GRID],
                                             _bad_rains("{d}/rain.tif:")),
    "order: a bad unit before the files": ({}, ["--rains", "{d}/small.tif", "--rain-unit", "x", "--grid", GRID], _bad("x")),
    "bad --rains: empty": ({}, ["--rains", "", "--grid", GRID], _bad_rains("")),
    "bad --rains: an empty member": ({}, ["--rains", "{d}/rain.tif::{d}/plain.tif", "--grid", GRID],
                                     _bad_rains("{d}/rain.tif::{d}/plain.tif")),
    "bad --rains: an empty first member": ({}, ["--rains", ":{d}/rain.tif", "--grid", GRID], _bad_rains(":{d}/rain.tif")),
    "bad --rains: a trailing colon": ({}, ["--rains", R + ":", "--grid", GRID], _bad_rains(R + ":")),
    "bad --rains: nine files": ({}, ["--rains", NINE, "--grid", GRID], _bad_rains(NINE)),
    "bad rains key: nine files": (dict(rains="a:b:c:d:e:f:g:h:i", grid=GRID), [], _bad_rains("a:b:c:d:e:f:g:h:i")),
    "bad --rains over a good key": (dict(rains=R, grid=GRID), ["--rains", "::"], _bad_rains("::")),
    "bad --rain-unit": ({}, ["--rains", R, "--rain-unit", "2.55", "--grid", GRID], _bad("2.55")),
    "wrong size, the second file": ({}, ["--rains", "{d}/rain.tif:{d}/small.tif", "--grid", GRID],
                                    "[rank 0] rains: '{d}/small.tif' has 29 x 22 pixels, the grid has 30 x 22 cells\n"),
    "wrong size, key, one file": (dict(rains="{d}/small.tif", grid=GRID), [],
                                  "[rank 0] rains: '{d}/small.tif' has 29 x 22 pixels, the grid has 30 x 22 cells\n"),
    "wrong geotransform, the third file": ({}, ["--rains", R + ":{d}/off.tif:{d}/small.tif", "--grid", GRID,
                                                "--rain-unit", "2"],
                                           "[rank 0] rains: '{d}/off.tif' does not lie on the grid (origin 10, "
                                           "50.000500000000002, pixel 0.0020999999999999999 x -0.0020999999999999999)\n"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refused_before_any_gpu(tmp_path, zones, rain, case):  # noqa: F811
    keys, args, stderr = REFUSALS[case]
    fill = dict(zones=zones, d=rain)
    args = [a.format(**fill) for a in args]
    keys = {k: v.format(**fill) if isinstance(v, str) else v for k, v in keys.items()}
    p = _gcn10(["-c", _config(tmp_path, **keys)] + args, tmp_path)
    assert p.returncode == 1, p.stdout + p.stderr
    assert p.stderr == stderr.format(**fill)
    assert p.stdout == ""
    assert _nothing_written(tmp_path)


def test_an_unreadable_file_is_refused_with_the_readers_message(tmp_path, rain):  # noqa: F811
    (tmp_path / "text.tif").write_text("no tiff at all, but long enough to hold a header\n" * 4)
    for name in ("nothing.tif", "text.tif"):
        path = str(tmp_path / name)
        p = _gcn10(["-c", _config(tmp_path), "--grid", GRID, "--rains", rain + "/rain.tif:" + path], tmp_path)
        assert p.returncode == 1, p.stdout + p.stderr
        assert p.stderr.startswith("[rank 0] rains: cannot read '%s': " % path) and p.stderr.count("\n") == 1
        assert len(p.stderr) > len("[rank 0] rains: cannot read '%s': \n" % path)
        assert p.stdout == "" and _nothing_written(tmp_path)


# ---- a GPU library without the entry points: the stub has none of the grid's -------------------------------------------

@pytest.mark.parametrize("how", ["flag", "key", "flag over key", "one file", "eight files"])
def test_a_gpu_library_without_the_rains_entry_points_fails_at_start(tmp_path, stub, rain, how):  # noqa: F811
    value = {"one file": rain + "/plain.tif", "eight files": ":".join([rain + "/rain.tif", rain + "/plain.tif"] * 4)}.get(
        how, rain + "/rain.tif:" + rain + "/plain.tif")
    keys = dict(grid=GRID, rains=value, rain_unit="2.5,0.1") if how == "key" else \
        dict(rains=rain + "/small.tif") if how == "flag over key" else {}
    args = [] if how == "key" else ["--grid", GRID, "--rains", value]
    p = _gcn10(["-c", _config(tmp_path, **keys)] + args, tmp_path, {"GCN10_GPU_LIB": stub})
    assert p.returncode == 1, p.stdout + p.stderr
    assert p.stderr == "[rank 0] %s lacks gcn10_gpu_grid_sums_rains (needed by rains=%s)\n" % (stub, value)
    assert p.stdout == ""
    assert _nothing_written(tmp_path)


def test_a_run_with_rain_alone_asks_for_the_rain_calls_as_before(tmp_path, stub, rain):  # noqa: F811
    path = rain + "/rain.tif"
    p = _gcn10(["-c", _config(tmp_path), "--grid", GRID, "--rain", path], tmp_path, {"GCN10_GPU_LIB": stub})
    assert p.returncode == 1
    assert p.stderr == "[rank 0] %s lacks gcn10_gpu_grid_sums_rain (needed by rain=%s)\n" % (stub, path)
