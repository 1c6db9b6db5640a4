"""CPU: every way a zonal run with several rainfall rasters (config key zone_rains, --zone-rains) stops before a GPU is
opened: exit status 1, the exact text on stderr, nothing created -- run the way tests/test_zone_rain_refusals.py runs its
table --; the order in which the refusals are tested; an unreadable second file; then the start-up failure on a GPU
library that lacks the entry point (the stub of tests/stub_gpu), and that a zonal run without the key, and a --zone-rain
run, ask for nothing new."""
import numpy as np
import pytest

from tests import tiffutil
from tests.test_grid_refusals import GRID, _config, _gcn10, _nothing_written, stub, zones  # noqa: F401

BAD = "(unit[,lambda]: 0 < unit, 255 unit <= 650 mm, 0 <= lambda < 1)"
BAD_LIST = "(file1[:file2...]: 1 to 8 files)"
GT = [9.9995, 0.0021, 0.0, 50.0005, 0.0, -0.0021]
OFF = [9.9995, 0.0021, 0.0, float(np.nextafter(50.0005, 60.0)), 0.0, -0.0021]


def _bad(text, rank=True):
    return "%sbad value for zone_rain_unit: '%s' %s\n" % ("[rank 0] " if rank else "", text, BAD)


def _bad_list(text):
    return "[rank 0] bad value for zone_rains: '%s' %s\n" % (text, BAD_LIST)


@pytest.fixture(scope="module")
def rain(tmp_path_factory):
    """atlas.tif and second.tif on one grid; plain.tif without a geotransform; south.tif not north up; wide.tif of another
    size; off.tif one unit in the last place north of atlas.tif"""
    tmp_path = tmp_path_factory.mktemp("zone_rains")
    f = np.random.default_rng(4).integers(0, 256, (22, 30)).astype(np.uint8)
    tiffutil.write_tiff(str(tmp_path / "atlas.tif"), f, gt=GT, compression=8, tile=(16, 16))
    tiffutil.write_tiff(str(tmp_path / "second.tif"), f[::-1].copy(), gt=GT)
    tiffutil.write_tiff(str(tmp_path / "plain.tif"), f)
    tiffutil.write_tiff(str(tmp_path / "south.tif"), f, gt=[9.9995, 0.0021, 0.0, 50.0005, 0.0, 0.0021])
    tiffutil.write_tiff(str(tmp_path / "wide.tif"), np.zeros((22, 31), np.uint8), gt=GT)
    tiffutil.write_tiff(str(tmp_path / "off.tif"), f, gt=OFF)
    return str(tmp_path)


A = ["--zone-rains", "{d}/atlas.tif:{d}/second.tif"]
ONE = ["--zone-rains", "{d}/atlas.tif"]
Z = ["--zones", "{zones}"]
NINE = ":".join(["{d}/atlas.tif"] * 9)
TOGETHER = "[rank 0] zone_rains cannot be combined with zone_rain\n"
# name -> (config keys, arguments behind "-c <config>", stderr)
REFUSALS = {
    # 1. the unit without either key: the text is unchanged
    "unit without either key": ({}, ["--zone-rain-unit", "2"] + Z, "[rank 0] zone_rain_unit needs zone_rain\n"),
    # 2. both keys
    "with --zone-rain": ({}, A + Z + ["--zone-rain", "{d}/atlas.tif"], TOGETHER),
    "key with the zone_rain key": (dict(zone_rains="{d}/atlas.tif", zone_rain="{d}/atlas.tif", zonal=1,
                                        zones_shp_path="{zones}"), [], TOGETHER),
    "flag with the zone_rain key": (dict(zone_rain="{d}/atlas.tif"), ONE + Z, TOGETHER),
    # 3. no zones
    "zone_rains alone": ({}, A, "[rank 0] zone_rains needs --zones\n"),
    "zone_rains key alone": (dict(zone_rains="{d}/atlas.tif:{d}/second.tif", zone_rain_unit="2"), [],
                             "[rank 0] zone_rains needs --zones\n"),
    "zone_rains with --grid, no zones": ({}, A + ["--grid", GRID], "[rank 0] zone_rains needs --zones\n"),
    # 4. storm, then storms
    "with --storm": ({}, A + Z + ["--storm", "50"], "[rank 0] zone_rains cannot be combined with storm\n"),
    "key with the storm key": (dict(zone_rains="{d}/atlas.tif", zonal=1, zones_shp_path="{zones}", storm="50"), [],
                               "[rank 0] zone_rains cannot be combined with storm\n"),
    "with --storms": ({}, A + Z + ["--storms", "25:50"], "[rank 0] zone_rains cannot be combined with storms\n"),
    "with the storms key": (dict(storms="25:50"), A + Z, "[rank 0] zone_rains cannot be combined with storms\n"),
    # 5. the list
    "bad list: empty": ({}, ["--zone-rains", ""] + Z, _bad_list("")),
    "bad list: an empty member": ({}, ["--zone-rains", "{d}/atlas.tif::{d}/second.tif"] + Z,
                                  _bad_list("{d}/atlas.tif::{d}/second.tif")),
    "bad list: a colon at the end": ({}, ["--zone-rains", "{d}/atlas.tif:"] + Z, _bad_list("{d}/atlas.tif:")),
    "bad list: nine files": ({}, ["--zone-rains", NINE] + Z, _bad_list(NINE)),
    "bad list key": (dict(zone_rains=":{d}/atlas.tif", zonal=1, zones_shp_path="{zones}"), [], _bad_list(":{d}/atlas.tif")),
    # 6. the unit
    "bad unit: 2.55": ({}, A + Z + ["--zone-rain-unit", "2.55"], _bad("2.55")),
    "bad unit: lambda = 1": ({}, A + Z + ["--zone-rain-unit", "1,1"], _bad("1,1")),
    "bad unit key": (dict(zone_rains="{d}/atlas.tif", zone_rain_unit="1,1.5"), Z, _bad("1,1.5", rank=False)),
    # 7. the files, in order
    "no geotransform, first file": ({}, ["--zone-rains", "{d}/plain.tif:{d}/atlas.tif"] + Z,
                                    "[rank 0] zone_rains: '{d}/plain.tif' carries no geotransform\n"),
    "no geotransform, second file": ({}, ["--zone-rains", "{d}/atlas.tif:{d}/plain.tif"] + Z,
                                     "[rank 0] zone_rains: '{d}/plain.tif' carries no geotransform\n"),
    "south up, one file": ({}, ["--zone-rains", "{d}/south.tif"] + Z,
                           "[rank 0] zone_rains: '{d}/south.tif' is rotated or not north up\n"),
    "another size": ({}, ["--zone-rains", "{d}/atlas.tif:{d}/second.tif:{d}/wide.tif"] + Z,
                     "[rank 0] zone_rains: '{d}/wide.tif' has 31 x 22 pixels, '{d}/atlas.tif' has 30 x 22\n"),
    "another size, key": (dict(zone_rains="{d}/wide.tif:{d}/atlas.tif", zonal=1, zones_shp_path="{zones}"), [],
                          "[rank 0] zone_rains: '{d}/atlas.tif' has 30 x 22 pixels, '{d}/wide.tif' has 31 x 22\n"),
    "another grid": ({}, ["--zone-rains", "{d}/atlas.tif:{d}/off.tif"] + Z,
                     "[rank 0] zone_rains: '{d}/off.tif' does not lie on the grid of '{d}/atlas.tif' (origin %.17g, %.17g, "
                     "pixel %.17g x %.17g)\n" % (OFF[0], OFF[3], OFF[1], OFF[5])),
    "the files in order: the size of the second before the grid of the third": (
        {}, ["--zone-rains", "{d}/atlas.tif:{d}/wide.tif:{d}/off.tif"] + Z,
        "[rank 0] zone_rains: '{d}/wide.tif' has 31 x 22 pixels, '{d}/atlas.tif' has 30 x 22\n"),
    # the order of the seven
    "order: the unit without a key needs no zones": ({}, ["--zone-rain-unit", "x"], "[rank 0] zone_rain_unit needs zone_rain\n"),
    "order: both keys before no zones": ({}, A + ["--zone-rain", "{d}/atlas.tif"], TOGETHER),
    "order: no zones before storm": ({}, A + ["--storm", "50"], "[rank 0] zone_rains needs --zones\n"),
    "order: storm before storms": ({}, A + Z + ["--storm", "50", "--storms", "25:50"],
                                   "[rank 0] zone_rains cannot be combined with storm\n"),
    "order: storms before a bad list": ({}, ["--zone-rains", ""] + Z + ["--storms", "25:50"],
                                        "[rank 0] zone_rains cannot be combined with storms\n"),
    "order: a bad list before a bad unit": ({}, ["--zone-rains", "a::b", "--zone-rain-unit", "x"] + Z, _bad_list("a::b")),
    "order: a bad unit before the files": ({}, ["--zone-rains", "{d}/plain.tif", "--zone-rain-unit", "x"] + Z, _bad("x")),
    "order: rain with zones stays refused first": ({}, A + Z + ["--rain", "{d}/atlas.tif"],
                                                   "[rank 0] rain cannot be combined with --zonal\n"),
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


def test_an_unreadable_second_file_is_refused_with_the_readers_message(tmp_path, zones, rain):  # noqa: F811
    for name in ("nothing.tif", "text.tif"):
        (tmp_path / "text.tif").write_text("no tiff at all, but long enough to hold a header\n" * 4)
        path = str(tmp_path / name)
        p = _gcn10(["-c", _config(tmp_path), "--zones", zones, "--zone-rains", rain + "/atlas.tif:" + path], tmp_path)
        assert p.returncode == 1, p.stdout + p.stderr
        assert p.stderr.startswith("[rank 0] zone_rains: cannot read '%s': " % path) and p.stderr.count("\n") == 1
        assert len(p.stderr) > len("[rank 0] zone_rains: cannot read '%s': \n" % path)
        assert p.stdout == "" and _nothing_written(tmp_path)


@pytest.mark.parametrize("how", ["flag", "key", "flag over key"])
def test_a_gpu_library_without_the_entry_point_fails_at_start(tmp_path, stub, zones, rain, how):  # noqa: F811
    value = rain + "/atlas.tif:" + rain + "/second.tif"
    keys = dict(zonal=1, zones_shp_path=zones, zone_rains=value, zone_rain_unit="2.5,0.1") if how == "key" else \
        dict(zone_rains=rain + "/plain.tif") if how == "flag over key" else {}
    args = [] if how == "key" else ["--zones", zones, "--zone-rains", value]
    p = _gcn10(["-c", _config(tmp_path, **keys)] + args, tmp_path, {"GCN10_GPU_LIB": stub})
    assert p.returncode == 1, p.stdout + p.stderr
    assert p.stderr == "[rank 0] %s lacks gcn10_gpu_zonal_sums_rains (needed by zone_rains=%s)\n" % (stub, value)
    assert p.stdout == ""
    assert _nothing_written(tmp_path)


def test_one_file_asks_for_the_new_call_too(tmp_path, stub, zones, rain):  # noqa: F811
    """zone_rains always runs through gcn10_gpu_zonal_sums_rains, as rains does through its own calls"""
    value = rain + "/atlas.tif"
    p = _gcn10(["-c", _config(tmp_path), "--zones", zones, "--zone-rains", value], tmp_path, {"GCN10_GPU_LIB": stub})
    assert p.returncode == 1
    assert p.stderr == "[rank 0] %s lacks gcn10_gpu_zonal_sums_rains (needed by zone_rains=%s)\n" % (stub, value)


def test_runs_without_the_key_ask_for_nothing_new(tmp_path, stub, zones, rain):  # noqa: F811
    """the zonal run's own message, and the --zone-rain run's, as before"""
    p = _gcn10(["-c", _config(tmp_path), "--zones", zones], tmp_path, {"GCN10_GPU_LIB": stub})
    assert p.returncode == 1
    assert p.stderr == "[rank 0] %s lacks gcn10_gpu_zonal_pair_histogram (needed by zonal=1)\n" % stub
    path = rain + "/atlas.tif"
    p = _gcn10(["-c", _config(tmp_path), "--zones", zones, "--zone-rain", path], tmp_path, {"GCN10_GPU_LIB": stub})
    assert p.returncode == 1
    assert p.stderr == "[rank 0] %s lacks gcn10_gpu_zonal_sums_rain (needed by zone_rain=%s)\n" % (stub, path)
