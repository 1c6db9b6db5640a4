"""CPU: every way a run with a rainfall raster (config keys rain / rain_unit, --rain / --rain-unit) stops before a GPU is
opened: exit status 1, the exact text on stderr, nothing created -- run the way tests/test_storm_refusals.py runs its
table --; the order in which the refusals are tested; then the start-up failure on a GPU library that lacks the entry
points (the stub of tests/stub_gpu), and that a run without rain asks for none of them."""
import numpy as np
import pytest

from tests import tiffutil
from tests.test_grid_refusals import GRID, _config, _gcn10, _nothing_written, stub, zones  # noqa: F401

BAD = "(unit[,lambda]: 0 < unit, 255 unit <= 650 mm, 0 <= lambda < 1)"
NX, NY = 30, 22
GT = [9.9995, 0.0021, 0.0, 50.0005, 0.0, -0.0021]


def _bad(text, rank=True):
    return "%sbad value for rain_unit: '%s' %s\n" % ("[rank 0] " if rank else "", text, BAD)


@pytest.fixture()
def rain(tmp_path):
    """rain.tif on GRID, small.tif of another size, off.tif beside the grid, plain.tif without georeferencing"""
    f = np.random.default_rng(4).integers(0, 256, (NY, NX)).astype(np.uint8)
    tiffutil.write_tiff(str(tmp_path / "rain.tif"), f, gt=GT, compression=8, tile=(16, 16))
    tiffutil.write_tiff(str(tmp_path / "small.tif"), f[:, :-1], gt=GT)
    tiffutil.write_tiff(str(tmp_path / "off.tif"), f, gt=[10.0, 0.0021, 0.0, 50.0005, 0.0, -0.0021])
    tiffutil.write_tiff(str(tmp_path / "plain.tif"), f)
    return str(tmp_path)


# name -> (config keys, arguments behind "-c <config>", stderr); "{zones}" stands for the zone file, "{d}" for the folder
# of the rasters above; a message without "[rank 0] " comes from the config parser, as it words it
REFUSALS = {
    "rain_unit without rain": ({}, ["--rain-unit", "2", "--grid", GRID], "[rank 0] rain_unit needs rain\n"),
    "rain_unit key without rain": (dict(rain_unit="2,0.1", grid=GRID), [], "[rank 0] rain_unit needs rain\n"),
    "rain alone": ({}, ["--rain", "{d}/rain.tif"], "[rank 0] rain needs --grid\n"),
    "rain key alone": (dict(rain="{d}/rain.tif", rain_unit="2"), [], "[rank 0] rain needs --grid\n"),
    "rain with --storm": ({}, ["--rain", "{d}/rain.tif", "--grid", GRID, "--storm", "50"],
                          "[rank 0] rain cannot be combined with storm\n"),
    "rain key with the storm key": (dict(rain="{d}/rain.tif", grid=GRID, storm="50"), [],
                                    "[rank 0] rain cannot be combined with storm\n"),
    "rain with --storms": ({}, ["--rain", "{d}/rain.tif", "--grid", GRID, "--storms", "25:50"],
                           "[rank 0] rain cannot be combined with storms\n"),
    "rain with the storms key": (dict(storms="25:50", grid=GRID), ["--rain", "{d}/rain.tif"],
                                 "[rank 0] rain cannot be combined with storms\n"),
    "rain with --verify": ({}, ["--rain", "{d}/rain.tif", "--grid", GRID, "--verify"],
                           "[rank 0] rain cannot be combined with --verify\n"),
    "rain with --aggregate": ({}, ["--rain", "{d}/rain.tif", "--grid", GRID, "--aggregate", "25"],
                              "[rank 0] rain cannot be combined with aggregate\n"),
    "rain key with aggregate=7": (dict(rain="{d}/rain.tif", aggregate=7), [],
                                  "[rank 0] rain cannot be combined with aggregate\n"),
    "rain with --zonal": ({}, ["--rain", "{d}/rain.tif", "--zones", "{zones}"],
                          "[rank 0] rain cannot be combined with --zonal\n"),
    "rain key with zonal=1": (dict(rain="{d}/rain.tif", zonal=1, zones_shp_path="{zones}", grid=GRID), [],
                              "[rank 0] rain cannot be combined with --zonal\n"),
    # the order: verify, aggregate, zonal, storm / storms, no grid
    "order: verify first": ({}, ["--rain", "{d}/rain.tif", "--verify", "--aggregate", "25", "--zones", "{zones}",
                                 "--storm", "50"], "[rank 0] rain cannot be combined with --verify\n"),
    "order: aggregate before zonal": ({}, ["--rain", "{d}/rain.tif", "--aggregate", "25", "--zones", "{zones}"],
                                      "[rank 0] rain cannot be combined with aggregate\n"),
    "order: zonal before storm": ({}, ["--rain", "{d}/rain.tif", "--zones", "{zones}", "--storm", "50"],
                                  "[rank 0] rain cannot be combined with --zonal\n"),
    "order: storm before no grid": ({}, ["--rain", "{d}/rain.tif", "--storm", "50"],
                                    "[rank 0] rain cannot be combined with storm\n"),
    "order: storms before no grid": ({}, ["--rain", "{d}/rain.tif", "--storms", "25:50"],
                                     "[rank 0] rain cannot be combined with storms\n"),
    "bad --rain-unit: empty": ({}, ["--rain", "{d}/rain.tif", "--rain-unit", "", "--grid", GRID], _bad("")),
    "bad --rain-unit: 2.55": ({}, ["--rain", "{d}/rain.tif", "--rain-unit", "2.55", "--grid", GRID], _bad("2.55")),
    "bad --rain-unit: 0": ({}, ["--rain", "{d}/rain.tif", "--rain-unit", "0", "--grid", GRID], _bad("0")),
    "bad --rain-unit: lambda = 1": ({}, ["--rain", "{d}/rain.tif", "--rain-unit", "1,1", "--grid", GRID], _bad("1,1")),
    "bad --rain-unit: text behind it": ({}, ["--rain", "{d}/rain.tif", "--rain-unit", "1mm", "--grid", GRID], _bad("1mm")),
    "bad --rain-unit over a good key": (dict(rain="{d}/rain.tif", rain_unit="2", grid=GRID), ["--rain-unit", "x"], _bad("x")),
    "bad rain_unit key": (dict(rain="{d}/rain.tif", rain_unit="1,1.5", grid=GRID), [], _bad("1,1.5", rank=False)),
    "bad rain_unit key under a good flag": (dict(rain="{d}/rain.tif", rain_unit="3", grid=GRID), ["--rain-unit", "1"],
                                            _bad("3", rank=False)),
    "wrong size": ({}, ["--rain", "{d}/small.tif", "--grid", GRID],
                   "[rank 0] rain: '{d}/small.tif' has 29 x 22 pixels, the grid has 30 x 22 cells\n"),
    "wrong size, key": (dict(rain="{d}/small.tif", grid=GRID), [],
                        "[rank 0] rain: '{d}/small.tif' has 29 x 22 pixels, the grid has 30 x 22 cells\n"),
    "wrong geotransform": ({}, ["--rain", "{d}/off.tif", "--grid", GRID, "--rain-unit", "2"],
                           "[rank 0] rain: '{d}/off.tif' does not lie on the grid (origin 10, 50.000500000000002, pixel "
                           "0.0020999999999999999 x -0.0020999999999999999)\n"),
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


def test_an_unreadable_file_is_refused_with_the_readers_message(tmp_path, rain):
    for name in ("nothing.tif", "text.tif"):
        (tmp_path / "text.tif").write_text("no tiff at all, but long enough to hold a header\n" * 4)
        path = str(tmp_path / name)
        p = _gcn10(["-c", _config(tmp_path), "--grid", GRID, "--rain", path], tmp_path)
        assert p.returncode == 1, p.stdout + p.stderr
        assert p.stderr.startswith("[rank 0] rain: cannot read '%s': " % path) and p.stderr.count("\n") == 1
        assert len(p.stderr) > len("[rank 0] rain: cannot read '%s': \n" % path)
        assert p.stdout == "" and _nothing_written(tmp_path)


# ---- a GPU library without the entry points: the stub has none of the grid's -------------------------------------------

@pytest.mark.parametrize("how", ["flag", "key", "flag over key", "without georeferencing"])
def test_a_gpu_library_without_the_rain_entry_points_fails_at_start(tmp_path, stub, rain, how):  # noqa: F811
    path = rain + ("/plain.tif" if how == "without georeferencing" else "/rain.tif")
    keys = dict(grid=GRID, rain=path, rain_unit="2.5,0.1") if how == "key" else \
        dict(rain=rain + "/small.tif") if how == "flag over key" else {}
    args = [] if how == "key" else ["--grid", GRID, "--rain", path]
    p = _gcn10(["-c", _config(tmp_path, **keys)] + args, tmp_path, {"GCN10_GPU_LIB": stub})
    assert p.returncode == 1, p.stdout + p.stderr
    assert p.stderr == "[rank 0] %s lacks gcn10_gpu_grid_sums_rain (needed by rain=%s)\n" % (stub, path)
    assert p.stdout == ""
    assert _nothing_written(tmp_path)


def test_a_run_without_rain_asks_for_none_of_them(tmp_path, stub):  # noqa: F811
    """the grid run's own message, as tests/test_grid_refusals.py pins it"""
    p = _gcn10(["-c", _config(tmp_path), "--grid", GRID], tmp_path, {"GCN10_GPU_LIB": stub})
    assert p.returncode == 1 and p.stderr == "[rank 0] %s lacks gcn10_gpu_grid_sums (needed by grid=%s)\n" % (stub, GRID)
