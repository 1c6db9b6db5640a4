"""CPU: every way a runoff_rain run (config keys runoff_rain, runoff_rain_unit, runoff_unit; --runoff-rain ...) stops
before a GPU is opened: exit status 1, one line on stderr, nothing created; the order in which the refusals are tested
(include/gcn10_host.h, "Runoff rasters under a rainfall raster"); the loader's four messages under the new prefix, and
unchanged under zone_rain; the start-up failure on a GPU library that lacks the entry points (the stub of
tests/stub_gpu), and that a plain run asks for nothing new."""
import os

import numpy as np
import pytest

from gcn10_amd import host
from tests import tiffutil
from tests.test_grid_refusals import GRID, _config, _gcn10, stub, zones  # noqa: F401

BAD_RAIN = "(unit[,lambda]: 0 < unit, 255 unit <= 650 mm, 0 <= lambda < 1)"
BAD_UNIT = "(millimetres per count, 0.01 to 650)"
GT = [9.9995, 0.0021, 0.0, 50.0005, 0.0, -0.0021]
WITH = "[rank 0] runoff_rain cannot be combined with %s\n"


@pytest.fixture(scope="module")
def rain(tmp_path_factory):
    """atlas.tif; plain.tif without a geotransform; south.tif not north up"""
    tmp_path = tmp_path_factory.mktemp("runoff_rain")
    f = np.random.default_rng(4).integers(0, 256, (22, 30)).astype(np.uint8)
    tiffutil.write_tiff(str(tmp_path / "atlas.tif"), f, gt=GT, compression=8, tile=(16, 16))
    tiffutil.write_tiff(str(tmp_path / "plain.tif"), f)
    tiffutil.write_tiff(str(tmp_path / "south.tif"), f, gt=[9.9995, 0.0021, 0.0, 50.0005, 0.0, 0.0021])
    return str(tmp_path)


def _nothing_written(tmp_path):
    return not (tmp_path / "logs").exists() and not [f for f in os.listdir(tmp_path)
                                                     if f.startswith("cn_") or f.startswith("runoff_")]


R = ["--runoff-rain", "{d}/atlas.tif"]
Z = ["--zones", "{zones}"]
# name -> (config keys, arguments behind "-c <config>", stderr); the refusals in the order they are tested
REFUSALS = {
    "unit without the key": ({}, ["--runoff-rain-unit", "2"], "[rank 0] runoff_rain_unit needs runoff_rain\n"),
    "unit key without the key": (dict(runoff_rain_unit="2"), [], "[rank 0] runoff_rain_unit needs runoff_rain\n"),
    "output unit without the key": ({}, ["--runoff-unit", "2"], "[rank 0] runoff_unit needs runoff_rain\n"),
    "output unit key without the key": (dict(runoff_unit="2"), [], "[rank 0] runoff_unit needs runoff_rain\n"),
    "with --verify": ({}, R + ["--verify"], WITH % "--verify"),
    "with the verify key": (dict(verify=1, runoff_rain="{d}/atlas.tif"), [], WITH % "--verify"),
    "with --aggregate": ({}, R + ["--aggregate", "25"], WITH % "aggregate"),
    "with the aggregate key": (dict(aggregate=7), R, WITH % "aggregate"),
    "with --zones": ({}, R + Z, WITH % "--zonal"),
    "with --zonal": ({}, R + ["--zonal"], WITH % "--zonal"),
    "with the zonal key": (dict(zonal=1, zones_shp_path="{zones}"), R, WITH % "--zonal"),
    "with --grid": ({}, R + ["--grid", GRID], WITH % "grid"),
    "with the grid key": (dict(grid=GRID, runoff_rain="{d}/atlas.tif"), [], WITH % "grid"),
    "with --storm": ({}, R + ["--storm", "50"], WITH % "storm"),
    "with the storm key": (dict(storm="50"), R, WITH % "storm"),
    "with --storms": ({}, R + ["--storms", "25:50"], WITH % "storms"),
    "with the storms key": (dict(storms="25:50"), R, WITH % "storms"),
    "with --rain": ({}, R + ["--rain", "{d}/atlas.tif"], WITH % "rain"),
    "with the rain key": (dict(rain="{d}/atlas.tif"), R, WITH % "rain"),
    "with --rains": ({}, R + ["--rains", "{d}/atlas.tif"], WITH % "rains"),
    "with the rains key": (dict(rains="{d}/atlas.tif"), R, WITH % "rains"),
    "with --zone-rain": ({}, R + ["--zone-rain", "{d}/atlas.tif"], WITH % "zone_rain"),
    "with the zone_rain key": (dict(zone_rain="{d}/atlas.tif"), R, WITH % "zone_rain"),
    "with --zone-rains": ({}, R + ["--zone-rains", "{d}/atlas.tif"], WITH % "zone_rains"),
    "with the zone_rains key": (dict(zone_rains="{d}/atlas.tif"), R, WITH % "zone_rains"),
    "with --cog": ({}, R + ["--cog"], WITH % "cog"),
    "with the cog key": (dict(cog=1), R, WITH % "cog"),
    "with --stats": ({}, R + ["--stats"], WITH % "stats"),
    "with the stats key": (dict(stats=1), R, WITH % "stats"),
    # the values
    "bad rain unit: 2.56": ({}, R + ["--runoff-rain-unit", "2.56"],
                            "[rank 0] bad value for runoff_rain_unit: '2.56' %s\n" % BAD_RAIN),
    "bad rain unit: lambda = 1": ({}, R + ["--runoff-rain-unit", "1,1"],
                                  "[rank 0] bad value for runoff_rain_unit: '1,1' %s\n" % BAD_RAIN),
    "bad rain unit key": (dict(runoff_rain_unit="x"), R, "bad value for runoff_rain_unit: 'x' %s\n" % BAD_RAIN),
    "bad output unit": ({}, R + ["--runoff-unit", "0"], "[rank 0] bad value for runoff_unit: '0' %s\n" % BAD_UNIT),
    "bad output unit: 651": ({}, R + ["--runoff-unit", "651"], "[rank 0] bad value for runoff_unit: '651' %s\n" % BAD_UNIT),
    "bad output unit key": (dict(runoff_unit="1,2"), R, "bad value for runoff_unit: '1,2' %s\n" % BAD_UNIT),
    # the raster
    "no geotransform": ({}, ["--runoff-rain", "{d}/plain.tif"], "[rank 0] runoff_rain: '{d}/plain.tif' carries no geotransform\n"),
    "no geotransform, key": (dict(runoff_rain="{d}/plain.tif"), [],
                             "[rank 0] runoff_rain: '{d}/plain.tif' carries no geotransform\n"),
    "south up": ({}, ["--runoff-rain", "{d}/south.tif"], "[rank 0] runoff_rain: '{d}/south.tif' is rotated or not north up\n"),
    # the order
    "order: the unit without the key before everything": ({}, ["--runoff-rain-unit", "x", "--verify", "--cog"],
                                                          "[rank 0] runoff_rain_unit needs runoff_rain\n"),
    "order: the rain unit before the output unit": ({}, ["--runoff-rain-unit", "1", "--runoff-unit", "1"],
                                                    "[rank 0] runoff_rain_unit needs runoff_rain\n"),
    "order: verify before aggregate": ({}, R + ["--verify", "--aggregate", "25"], WITH % "--verify"),
    "order: aggregate before zones": ({}, R + ["--aggregate", "25"] + Z, WITH % "aggregate"),
    "order: zones before grid": ({}, R + Z + ["--grid", GRID], WITH % "--zonal"),
    "order: grid before storm": ({}, R + ["--grid", GRID, "--storm", "50"], WITH % "grid"),
    "order: storm before storms": ({}, R + ["--storm", "50", "--storms", "25:50"], WITH % "storm"),
    "order: storms before rain": ({}, R + ["--storms", "25:50", "--rain", "{d}/atlas.tif"], WITH % "storms"),
    "order: rain before rains": ({}, R + ["--rain", "{d}/atlas.tif", "--rains", "{d}/atlas.tif"], WITH % "rain"),
    "order: rains before zone_rain": ({}, R + ["--rains", "{d}/atlas.tif", "--zone-rain", "{d}/atlas.tif"], WITH % "rains"),
    "order: zone_rain before zone_rains": ({}, R + ["--zone-rain", "{d}/atlas.tif", "--zone-rains", "{d}/atlas.tif"],
                                           WITH % "zone_rain"),
    "order: zone_rains before cog": ({}, R + ["--zone-rains", "{d}/atlas.tif", "--cog"], WITH % "zone_rains"),
    "order: cog before stats": ({}, R + ["--cog", "--stats"], WITH % "cog"),
    "order: stats before a bad unit": ({}, R + ["--stats", "--runoff-rain-unit", "x"], WITH % "stats"),
    "order: a bad rain unit before a bad output unit": ({}, R + ["--runoff-rain-unit", "x", "--runoff-unit", "x"],
                                                        "[rank 0] bad value for runoff_rain_unit: 'x' %s\n" % BAD_RAIN),
    "order: a bad output unit before the raster": ({}, ["--runoff-rain", "{d}/plain.tif", "--runoff-unit", "x"],
                                                   "[rank 0] bad value for runoff_unit: 'x' %s\n" % BAD_UNIT),
    "order: rain alone stays what it was": ({}, ["--rain", "{d}/atlas.tif"], "[rank 0] rain needs --grid\n"),
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


def test_an_unreadable_raster_is_refused_with_the_readers_message(tmp_path):
    for name in ("nothing.tif", "text.tif"):
        (tmp_path / "text.tif").write_text("no tiff at all, but long enough to hold a header\n" * 4)
        path = str(tmp_path / name)
        p = _gcn10(["-c", _config(tmp_path), "--runoff-rain", path], tmp_path)
        assert p.returncode == 1, p.stdout + p.stderr
        assert p.stderr.startswith("[rank 0] runoff_rain: cannot read '%s': " % path) and p.stderr.count("\n") == 1
        assert len(p.stderr) > len("[rank 0] runoff_rain: cannot read '%s': \n" % path)
        assert p.stdout == "" and _nothing_written(tmp_path)


def test_the_loaders_four_messages_under_either_prefix(tmp_path, rain, monkeypatch):
    """cannot read, no geotransform, not north up, too many pixels -- and zone_rain prints what it printed"""
    huge = str(tmp_path / "huge.tif")
    tiffutil.write_tiff(huge, np.zeros((8193, 8192), np.uint8), gt=GT, compression=8, tile=(256, 256))
    cases = [(str(tmp_path / "nothing.tif"), "cannot read '%s': "), (rain + "/plain.tif", "'%s' carries no geotransform"),
             (rain + "/south.tif", "'%s' is rotated or not north up"), (huge, "'%s' has more than 67108864 pixels")]
    for path, text in cases:
        for prefix in ("runoff_rain", "zone_rain"):
            with pytest.raises(host.HostError) as e:
                host.rain_raster_load(prefix, path)
            assert str(e.value).startswith(prefix + ": " + text % path), str(e.value)
            if not text.endswith(": "):
                assert str(e.value) == prefix + ": " + text % path
        with pytest.raises(host.HostError) as e:
            host.zone_rain_load(path)
        with pytest.raises(host.HostError) as e2:
            host.rain_raster_load("zone_rain", path)
        assert str(e.value) == str(e2.value)
    grid, f = host.rain_raster_load("runoff_rain", rain + "/atlas.tif")
    grid2, f2 = host.zone_rain_load(rain + "/atlas.tif")
    assert grid == grid2 and (f == f2).all() and f.shape == (22, 30)


@pytest.mark.parametrize("how", ["flag", "key", "flag over key"])
def test_a_gpu_library_without_the_entry_points_fails_at_start(tmp_path, stub, rain, how):  # noqa: F811
    value = rain + "/atlas.tif"
    keys = dict(runoff_rain=value, runoff_rain_unit="2.5,0.1", runoff_unit="1") if how == "key" else \
        dict(runoff_rain=rain + "/plain.tif") if how == "flag over key" else {}
    args = [] if how == "key" else ["--runoff-rain", value]
    p = _gcn10(["-c", _config(tmp_path, **keys)] + args, tmp_path, {"GCN10_GPU_LIB": stub})
    assert p.returncode == 1, p.stdout + p.stderr
    assert p.stderr == "[rank 0] %s lacks gcn10_gpu_runoff_strip (needed by runoff_rain=%s)\n" % (stub, value)
    assert p.stdout == ""
    assert _nothing_written(tmp_path)


def test_the_keys_are_parsed(tmp_path, rain):
    cfg = host.parse_config(_config(tmp_path, runoff_rain=rain + "/atlas.tif", runoff_rain_unit="2.5,0.1", runoff_unit="0.5"))
    assert (cfg["runoff_rain"], cfg["runoff_rain_unit"], cfg["runoff_unit"]) == (rain + "/atlas.tif", "2.5,0.1", "0.5")
    cfg = host.parse_config(_config(tmp_path))
    assert cfg["runoff_rain"] is None and cfg["runoff_rain_unit"] is None and cfg["runoff_unit"] is None
