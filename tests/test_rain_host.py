"""CPU: the host side of the rainfall raster (config keys rain / rain_unit): gcn10_parse_rain_unit on good and bad
texts, the 256 tables of gcn10_rain_tables against tests/runoffutil.py::table, the size and geotransform checks of
gcn10_rain_load -- the compare is bit for bit, a file without georeferencing lies on the grid --, the config keys, the
numpy restatement of tests/rainutil.py against runoffutil.add_triples, and the parser and the table builder as a
stand-alone program under AddressSanitizer + UBSan (tests/rain_san_main.c)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from gcn10_amd import host
from tests import rainutil as rn
from tests import runoffutil as ru
from tests import tiffutil
from tests.conftest import ROOT

BASE = "hysogs_data_path=h\nesa_data_path=e\nblocks_shp_path=b\nlookup_table_path=l\nlog_dir=d\n"
GOOD = [("1", (1.0, 0.2)), ("2.5", (2.5, 0.2)), ("0.1,0", (0.1, 0.0)), ("2.5490196078431371,0.05", (2.5490196078431371, 0.05)),
        ("+.5,.999", (0.5, 0.999)), ("1e-3", (0.001, 0.2)), ("2,0.2", (2.0, 0.2))]
REFUSED = ["", " 1", "1 ", "x", "1,", ",0.2", "1,0.2,3", "1;0.2", "0", "-1", "2.55", "2.5490196078431376", "1e9", "nan",
           "inf", "1,nan", "1,1", "1,-0.1", "1,1.5", "1mm", "1, 0.2"]
GRID = dict(xmin=9.9995, ymax=50.0005, dx=0.0021, dy=0.0021, nx=30, ny=22)
GT = [GRID["xmin"], GRID["dx"], 0.0, GRID["ymax"], 0.0, -GRID["dy"]]


@pytest.mark.parametrize("text,want", GOOD)
def test_good_units(text, want):
    assert host.parse_rain_unit(text) == want
    assert 255.0 * want[0] <= 650.0


@pytest.mark.parametrize("text", REFUSED)
def test_refused_units(text):
    with pytest.raises(host.HostError, match="bad value for rain_unit"):
        host.parse_rain_unit(text)


def test_the_largest_unit_is_650_over_255_as_doubles():
    assert 255.0 * 2.5490196078431371 <= 650.0 < 255.0 * 2.5490196078431376


@pytest.mark.parametrize("unit,lam", [(1.0, 0.2), (2.5, 0.2), (0.1, 0.0), (2.5490196078431371, 0.05), (0.37, 0.999)])
def test_the_256_tables_are_the_runoff_tables_of_the_depths(unit, lam):
    q = host.rain_tables(unit, lam)
    assert q.shape == (256, 256) and q.dtype == np.uint16
    for b in range(256):
        np.testing.assert_array_equal(q[b], ru.table(b * unit, lam), err_msg="table %d" % b)
        np.testing.assert_array_equal(q[b], host.runoff_table(b * unit, lam) if b else np.zeros(256, np.uint16))
    assert not q[0].any() and q[:, 0].max() == 0 and q[:, 255].max() == 0
    assert (np.diff(q[:, 100].astype(np.int64)) >= 0).all() and q[255, 100] == round(25500 * unit)


def test_the_config_keys(tmp_path):
    (tmp_path / "c.txt").write_text(BASE)
    cfg = host.parse_config(str(tmp_path / "c.txt"))
    assert cfg["rain"] is None and cfg["rain_unit"] is None
    (tmp_path / "c.txt").write_text(BASE + "rain = /data/atlas.tif \nrain_unit=2.5,0.05\n")
    cfg = host.parse_config(str(tmp_path / "c.txt"))
    assert cfg["rain"] == "/data/atlas.tif" and cfg["rain_unit"] == "2.5,0.05" and cfg["storm"] is None
    for bad in ("3", "1,1", ""):
        (tmp_path / "c.txt").write_text(BASE + "rain=r.tif\nrain_unit=%s\n" % bad)
        with pytest.raises(host.HostError) as e:
            host.parse_config(str(tmp_path / "c.txt"))
        assert str(e.value) == "bad value for rain_unit: '%s' (unit[,lambda]: 0 < unit, 255 unit <= 650 mm, 0 <= " \
            "lambda < 1)" % bad
    assert [n for n, _t in host.ConfigRain._fields_] == ["rain", "rain_unit"] and issubclass(host.ConfigRain, host.ConfigStorms)


# ---- the raster: size and geotransform ----------------------------------------------------------------------------

def _field(seed=1):
    return np.random.default_rng(seed).integers(0, 256, (GRID["ny"], GRID["nx"])).astype(np.uint8)


@pytest.mark.parametrize("layout", [dict(), dict(compression=8, tile=(16, 16)), dict(compression=5, rows_per_strip=3),
                                    dict(compression=8, tile=(256, 256), predictor=2, bigtiff=True)])
def test_a_raster_on_the_grid_is_read_whole(tmp_path, layout):
    f = _field()
    path = str(tmp_path / "rain.tif")
    tiffutil.write_tiff(path, f, gt=GT, **layout)
    np.testing.assert_array_equal(host.rain_load(path, GRID), f)


def test_a_raster_without_georeferencing_lies_on_the_grid(tmp_path):
    f = _field(2)
    path = str(tmp_path / "plain.tif")
    tiffutil.write_tiff(path, f)
    np.testing.assert_array_equal(host.rain_load(path, GRID), f)


@pytest.mark.parametrize("shape", [(22, 29), (21, 30), (30, 22), (1, 1)])
def test_another_size_is_refused(tmp_path, shape):
    path = str(tmp_path / "small.tif")
    tiffutil.write_tiff(path, np.zeros(shape, np.uint8), gt=GT)
    with pytest.raises(host.HostError) as e:
        host.rain_load(path, GRID)
    assert str(e.value) == "rain: '%s' has %d x %d pixels, the grid has 30 x 22 cells" % (path, shape[1], shape[0])
    assert e.value.code == -2


@pytest.mark.parametrize("k,value", [(0, np.nextafter(GRID["xmin"], 100.0)), (3, np.nextafter(GRID["ymax"], 0.0)),
                                     (1, np.nextafter(GRID["dx"], 1.0)), (5, -np.nextafter(GRID["dy"], 0.0)),
                                     (0, 10.0)])
def test_a_geotransform_one_ulp_off_is_refused(tmp_path, k, value):
    gt = list(GT)
    gt[k] = float(value)
    path = str(tmp_path / "off.tif")
    tiffutil.write_tiff(path, _field(), gt=gt)
    with pytest.raises(host.HostError) as e:
        host.rain_load(path, GRID)
    assert str(e.value) == "rain: '%s' does not lie on the grid (origin %.17g, %.17g, pixel %.17g x %.17g)" % (
        path, gt[0], gt[3], gt[1], gt[5])
    assert e.value.code == -3


def test_an_unreadable_file_is_refused_with_the_readers_message(tmp_path):
    path = str(tmp_path / "none.tif")
    with pytest.raises(host.HostError) as e:
        host.rain_load(path, GRID)
    assert str(e.value).startswith("rain: cannot read '%s': " % path) and e.value.code == -1
    (tmp_path / "text.tif").write_text("no tiff at all, but long enough to hold a header\n" * 4)
    with pytest.raises(host.HostError) as e:
        host.rain_load(str(tmp_path / "text.tif"), GRID)
    assert str(e.value).startswith("rain: cannot read '%s': " % (tmp_path / "text.tif")) and e.value.code == -1


# ---- the restatement ----------------------------------------------------------------------------------------------

def test_add_triples_with_a_constant_field_adds_what_runoffutil_adds():
    from tests.test_gpu_grid import maps
    rng = np.random.default_rng(2)
    W, rows = 333, 77
    raster = rng.choice(np.array([0, 1, 77, 100, 254, 255], np.uint8), size=(rows, W))
    cellx, celly = maps(W, rows, 8.5, 17.3, (2, 1), (1, 2))
    ncx, ncy = int(cellx.max()) + 1, int(celly.max()) + 1
    tables = rn.tables_256()
    got = np.zeros((ncy, ncx, 3), np.int64)
    rn.add_triples(got, raster, cellx, celly, np.full((ncy, ncx), 9, np.uint8), tables)
    want = np.zeros_like(got)
    ru.add_triples(want, raster, cellx, celly, tables[9])
    np.testing.assert_array_equal(got, want)
    # a byte per cell: every cell alone is its own table's; a byte that names no table counts as table 0
    field = rng.integers(0, 256, (ncy, ncx)).astype(np.uint8)
    got[:] = 0
    rn.add_triples(got, raster, cellx, celly, field, tables[:100])
    for cy, cx in ((0, 0), (ncy - 1, ncx - 1), (2, 17)):
        one = np.zeros_like(got)
        b = int(field[cy, cx])
        ru.add_triples(one, raster, np.where(cellx == cx, cellx, -1), np.where(celly == cy, celly, -1),
                       tables[b if b < 100 else 0])
        np.testing.assert_array_equal(got[cy, cx], one[cy, cx])
    assert (field >= 100).any() and got[..., 2].max() > 0
    np.testing.assert_array_equal(rn.cn_cells(got.reshape(1, -1, 3), np.full(ncy * ncx, 9), tables)[0],
                                  ru.cn_array(got.reshape(-1, 3), tables[9]))


# ---- the parser and the table builder under the sanitizers ---------------------------------------------------------

def test_the_parser_and_the_tables_as_a_sanitized_program(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    exe = str(tmp_path / "rain_san")
    # both runtimes linked statically: the program then runs in any environment, whatever else is loaded before it
    cmd = [cc, "-std=c99", "-D_GNU_SOURCE", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "rain_san_main.c"),
           os.path.join(ROOT, "gcn10_amd", "csrc", "host", "runoff.c"), "-lm"]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(*args):
        p = subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=120)
        assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
        assert p.returncode in (0, 1), (args, p.returncode, p.stderr[-3000:])
        return p

    long_texts = ["9" * 400, "1," + "0" * 300 + ".5", "," * 300, "1," * 300, "1e400", "1e-400"]
    p = run(*(REFUSED + long_texts))
    lines = p.stdout.split("\n")[:-1]
    assert p.returncode == 1 and len(lines) == len(REFUSED) + len(long_texts)
    for text, line in zip(REFUSED + long_texts, lines):
        assert (line == "bad") == (text != "1," + "0" * 300 + ".5"), text
    good = "2.5490196078431371,0.05"
    prefixes = [good[:n] for n in range(len(good) + 1)]
    p = run(*prefixes)
    lines = p.stdout.split("\n")[:-1]
    assert len(lines) == len(prefixes)
    for text, line in zip(prefixes, lines):
        try:
            unit, lam = host.parse_rain_unit(text)
        except host.HostError:
            assert line == "bad", text
            continue
        q = np.stack([ru.table(b * unit, lam) for b in range(256)])
        assert line == "unit %.17g %.17g | %d %d %d %d %d" % (unit, lam, q[1, 100], q[128, 100], q[255, 100], q[255, 50],
                                                             int(q.astype(np.int64).sum())), text
    assert lines[0] == "bad" and sum(ln != "bad" for ln in lines) > 8
    for text, want in GOOD:
        p = run(text)
        assert p.returncode == 0 and p.stdout.startswith("unit %.17g %.17g | " % want), p.stdout
