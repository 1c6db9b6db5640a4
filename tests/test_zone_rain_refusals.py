"""CPU: every way a zonal run with a rainfall raster (config keys zone_rain / zone_rain_unit, --zone-rain /
--zone-rain-unit) stops before a GPU is opened: exit status 1, the exact text on stderr, nothing created -- run the way
tests/test_rain_refusals.py runs its table --; the order in which the refusals are tested; then the start-up failure
on a GPU library that lacks the entry point (the stub of tests/stub_gpu), and that a zonal run without the key asks for
nothing new."""
import numpy as np
import pytest

from tests import tiffutil
from tests.test_grid_refusals import GRID, _config, _gcn10, _nothing_written, stub, zones  # noqa: F401

BAD = "(unit[,lambda]: 0 < unit, 255 unit <= 650 mm, 0 <= lambda < 1)"
GT = [9.9995, 0.0021, 0.0, 50.0005, 0.0, -0.0021]


def _bad(text, rank=True):
    return "%sbad value for zone_rain_unit: '%s' %s\n" % ("[rank 0] " if rank else "", text, BAD)


@pytest.fixture(scope="module")
def rain(tmp_path_factory):
    """atlas.tif with a geotransform, plain.tif without, south.tif and mirror.tif not north up, big.tif too large"""
    tmp_path = tmp_path_factory.mktemp("zone_rain")
    f = np.random.default_rng(4).integers(0, 256, (22, 30)).astype(np.uint8)
    tiffutil.write_tiff(str(tmp_path / "atlas.tif"), f, gt=GT, compression=8, tile=(16, 16))
    tiffutil.write_tiff(str(tmp_path / "plain.tif"), f)
    tiffutil.write_tiff(str(tmp_path / "south.tif"), f, gt=[9.9995, 0.0021, 0.0, 50.0005, 0.0, 0.0021])
    tiffutil.write_tiff(str(tmp_path / "mirror.tif"), f, gt=[9.9995, -0.0021, 0.0, 50.0005, 0.0, -0.0021])
    tiffutil.write_tiff(str(tmp_path / "big.tif"), np.zeros((8193, 8192), np.uint8), gt=GT, compression=8)
    return str(tmp_path)


A = ["--zone-rain", "{d}/atlas.tif"]
Z = ["--zones", "{zones}"]
# name -> (config keys, arguments behind "-c <config>", stderr)
REFUSALS = {
    "unit without zone_rain": ({}, ["--zone-rain-unit", "2"] + Z, "[rank 0] zone_rain_unit needs zone_rain\n"),
    "unit key without zone_rain": (dict(zone_rain_unit="2,0.1", zonal=1, zones_shp_path="{zones}"), [],
                                   "[rank 0] zone_rain_unit needs zone_rain\n"),
    "zone_rain alone": ({}, A, "[rank 0] zone_rain needs --zones\n"),
    "zone_rain key alone": (dict(zone_rain="{d}/atlas.tif", zone_rain_unit="2"), [], "[rank 0] zone_rain needs --zones\n"),
    "zone_rain with --grid, no zones": ({}, A + ["--grid", GRID], "[rank 0] zone_rain needs --zones\n"),
    "with --storm": ({}, A + Z + ["--storm", "50"], "[rank 0] zone_rain cannot be combined with storm\n"),
    "key with the storm key": (dict(zone_rain="{d}/atlas.tif", zonal=1, zones_shp_path="{zones}", storm="50"), [],
                               "[rank 0] zone_rain cannot be combined with storm\n"),
    "with --storms": ({}, A + Z + ["--storms", "25:50"], "[rank 0] zone_rain cannot be combined with storms\n"),
    "with the storms key": (dict(storms="25:50"), A + Z, "[rank 0] zone_rain cannot be combined with storms\n"),
    # the order: the unit without the raster, no zones, storm, storms, the unit's value, the file
    "order: no zones before storm": ({}, A + ["--storm", "50"], "[rank 0] zone_rain needs --zones\n"),
    "order: storm before storms": ({}, A + Z + ["--storm", "50", "--storms", "25:50"],
                                   "[rank 0] zone_rain cannot be combined with storm\n"),
    "order: storms before a bad unit": ({}, A + Z + ["--storms", "25:50", "--zone-rain-unit", "x"],
                                        "[rank 0] zone_rain cannot be combined with storms\n"),
    "order: a bad unit before the file": ({}, ["--zone-rain", "{d}/plain.tif", "--zone-rain-unit", "x"] + Z, _bad("x")),
    "order: rain with zones stays refused first": ({}, A + Z + ["--rain", "{d}/atlas.tif"],
                                                   "[rank 0] rain cannot be combined with --zonal\n"),
    "bad unit: empty": ({}, A + Z + ["--zone-rain-unit", ""], _bad("")),
    "bad unit: 2.55": ({}, A + Z + ["--zone-rain-unit", "2.55"], _bad("2.55")),
    "bad unit: 0": ({}, A + Z + ["--zone-rain-unit", "0"], _bad("0")),
    "bad unit: lambda = 1": ({}, A + Z + ["--zone-rain-unit", "1,1"], _bad("1,1")),
    "bad unit: text behind it": ({}, A + Z + ["--zone-rain-unit", "1mm"], _bad("1mm")),
    "bad unit key": (dict(zone_rain="{d}/atlas.tif", zone_rain_unit="1,1.5"), Z, _bad("1,1.5", rank=False)),
    "no geotransform": ({}, ["--zone-rain", "{d}/plain.tif"] + Z,
                        "[rank 0] zone_rain: '{d}/plain.tif' carries no geotransform\n"),
    "no geotransform, key": (dict(zone_rain="{d}/plain.tif", zonal=1, zones_shp_path="{zones}"), [],
                             "[rank 0] zone_rain: '{d}/plain.tif' carries no geotransform\n"),
    "south up": ({}, ["--zone-rain", "{d}/south.tif"] + Z, "[rank 0] zone_rain: '{d}/south.tif' is rotated or not north up\n"),
    "mirrored": ({}, ["--zone-rain", "{d}/mirror.tif"] + Z,
                 "[rank 0] zone_rain: '{d}/mirror.tif' is rotated or not north up\n"),
    "too many pixels": ({}, ["--zone-rain", "{d}/big.tif"] + Z,
                        "[rank 0] zone_rain: '{d}/big.tif' has more than 67108864 pixels\n"),
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


def test_an_unreadable_file_is_refused_with_the_readers_message(tmp_path, zones):  # noqa: F811
    for name in ("nothing.tif", "text.tif"):
        (tmp_path / "text.tif").write_text("no tiff at all, but long enough to hold a header\n" * 4)
        path = str(tmp_path / name)
        p = _gcn10(["-c", _config(tmp_path), "--zones", zones, "--zone-rain", path], tmp_path)
        assert p.returncode == 1, p.stdout + p.stderr
        assert p.stderr.startswith("[rank 0] zone_rain: cannot read '%s': " % path) and p.stderr.count("\n") == 1
        assert len(p.stderr) > len("[rank 0] zone_rain: cannot read '%s': \n" % path)
        assert p.stdout == "" and _nothing_written(tmp_path)


@pytest.mark.parametrize("how", ["flag", "key", "flag over key"])
def test_a_gpu_library_without_the_entry_point_fails_at_start(tmp_path, stub, zones, rain, how):  # noqa: F811
    path = rain + "/atlas.tif"
    keys = dict(zonal=1, zones_shp_path=zones, zone_rain=path, zone_rain_unit="2.5,0.1") if how == "key" else \
        dict(zone_rain=rain + "/plain.tif") if how == "flag over key" else {}
    args = [] if how == "key" else ["--zones", zones, "--zone-rain", path]
    p = _gcn10(["-c", _config(tmp_path, **keys)] + args, tmp_path, {"GCN10_GPU_LIB": stub})
    assert p.returncode == 1, p.stdout + p.stderr
    assert p.stderr == "[rank 0] %s lacks gcn10_gpu_zonal_sums_rain (needed by zone_rain=%s)\n" % (stub, path)
    assert p.stdout == ""
    assert _nothing_written(tmp_path)


def test_a_zonal_run_without_the_key_asks_for_nothing_new(tmp_path, stub, zones):  # noqa: F811
    """the zonal run's own message, as before"""
    p = _gcn10(["-c", _config(tmp_path), "--zones", zones], tmp_path, {"GCN10_GPU_LIB": stub})
    assert p.returncode == 1
    assert p.stderr == "[rank 0] %s lacks gcn10_gpu_zonal_pair_histogram (needed by zonal=1)\n" % stub
