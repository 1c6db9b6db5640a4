"""CPU: the host side of several rainfall rasters in one run (config key rains): gcn10_parse_rains on good and bad
texts, gcn10_rains_load on fixtures written with tests/tiffutil.py -- every raster as written, the first bad file's
refusal under the prefix "rains:" --, the bytes of a shared cell per layer (gcn10_rains_cell) against runoffutil.cn, the
config key, and all three as a stand-alone program under AddressSanitizer + UBSan (tests/rains_san_main.c)."""
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

from gcn10_amd import host
from tests import runoffutil as ru
from tests import tiffutil
from tests.conftest import ROOT

BASE = "hysogs_data_path=h\nesa_data_path=e\nblocks_shp_path=b\nlookup_table_path=l\nlog_dir=d\n"
GRID = dict(xmin=9.9995, ymax=50.0005, dx=0.0021, dy=0.0021, nx=30, ny=22)
GRID_TEXT = "9.9995,50.0005,0.0021,0.0021,30,22"
GT = [GRID["xmin"], GRID["dx"], 0.0, GRID["ymax"], 0.0, -GRID["dy"]]
GOOD = [("a.tif", ["a.tif"]), ("a.tif:b.tif", ["a.tif", "b.tif"]), ("/x/y z.tif:rel/b,1.tif", ["/x/y z.tif", "rel/b,1.tif"]),
        (":".join("f%d" % j for j in range(8)), ["f%d" % j for j in range(8)]), ("a:a", ["a", "a"]), (" ", [" "])]
REFUSED = ["", ":", "a:", ":a", "a::b", "a:b:", "::", ":".join("f%d" % j for j in range(9)), ":".join("f" * 9) + ":"]


@pytest.mark.parametrize("text,want", GOOD)
def test_good_lists(text, want):
    assert host.parse_rains(text) == want and 1 <= len(want) <= host.MAX_RAINS == 8


@pytest.mark.parametrize("text", REFUSED)
def test_refused_lists(text):
    with pytest.raises(host.HostError, match="bad value for rains"):
        host.parse_rains(text)


def test_the_config_key(tmp_path):
    p = tmp_path / "cfg.txt"
    p.write_text(BASE)
    assert host.parse_config(str(p))["rains"] is None
    p.write_text(BASE + "rains=a.tif:b.tif\nrain_unit=2,0.1\n")
    cfg = host.parse_config(str(p))
    assert cfg["rains"] == "a.tif:b.tif" and cfg["rain_unit"] == "2,0.1" and cfg["rain"] is None


@pytest.fixture()
def rasters(tmp_path):
    """three rasters on GRID (one without georeferencing, one tiled and compressed), one of another size, one beside
    the grid"""
    rng = np.random.default_rng(14)
    f = rng.integers(0, 256, (3, GRID["ny"], GRID["nx"])).astype(np.uint8)
    tiffutil.write_tiff(str(tmp_path / "r1.tif"), f[0], gt=GT, compression=8, tile=(16, 16))
    tiffutil.write_tiff(str(tmp_path / "r2.tif"), f[1])
    tiffutil.write_tiff(str(tmp_path / "r3.tif"), f[2], gt=GT)
    tiffutil.write_tiff(str(tmp_path / "small.tif"), f[0][:, :-1], gt=GT)
    tiffutil.write_tiff(str(tmp_path / "off.tif"), f[0], gt=[10.0, 0.0021, 0.0, 50.0005, 0.0, -0.0021])
    return str(tmp_path), f


def test_every_raster_is_loaded_as_written_in_the_order_given(rasters):
    d, f = rasters
    got = host.rains_load([d + "/r3.tif", d + "/r1.tif", d + "/r2.tif", d + "/r1.tif"], GRID)
    np.testing.assert_array_equal(got, f[[2, 0, 1, 0]])
    np.testing.assert_array_equal(host.rains_load([d + "/r2.tif"], GRID)[0], host.rain_load(d + "/r2.tif", GRID))


@pytest.mark.parametrize("bad,code,text", [
    ("small.tif", -2, "rains: '%s' has 29 x 22 pixels, the grid has 30 x 22 cells"),
    ("off.tif", -3, "rains: '%s' does not lie on the grid (origin 10, 50.000500000000002, pixel 0.0020999999999999999 x "
                    "-0.0020999999999999999)"),
    ("none.tif", -1, "rains: cannot read '%s': ")])
def test_the_first_bad_file_is_refused_with_the_prefix_rains(rasters, bad, code, text):
    d, _ = rasters
    for files in ([d + "/" + bad], [d + "/r1.tif", d + "/r2.tif", d + "/" + bad, d + "/small.tif"]):
        with pytest.raises(host.HostError) as e:
            host.rains_load(files, GRID)
        want = text % (d + "/" + bad)
        assert e.value.code == code and (str(e.value) == want or (code == -1 and str(e.value).startswith(want)))
        # what gcn10_rain_load says of the same file, under the other prefix
        with pytest.raises(host.HostError) as one:
            host.rain_load(d + "/" + bad, GRID)
        assert str(e.value) == "rains" + str(one.value)[len("rain"):]


def test_the_bytes_of_a_cell_per_layer_are_the_cell_rule_with_the_layers_table():
    q = host.rain_tables(2.5, 0.05)
    rng = np.random.default_rng(21)
    for k in (1, 2, 3, 8):
        for _ in range(40):
            n = int(rng.integers(0, 5000))
            s = int(rng.integers(0, 100 * n + 1))
            b = rng.integers(0, 256, k).astype(np.uint8)
            b[rng.integers(0, k)] = 0
            sw = [int(n * int(q[b[j]][int(rng.integers(1, 101))]) + rng.integers(0, 2)) * int(rng.integers(0, 4) > 0)
                  for j in range(k)]
            got = host.rains_cell([s, n] + sw, b, q)
            assert got == [ru.cn(s, n, sw[j], q[b[j]]) for j in range(k)]
            assert got == [host.runoff_cn(s, n, sw[j], q[b[j]]) for j in range(k)]


# ---- the parser, the loader and the cell rule under AddressSanitizer + UBSan ------------------------------------------

def test_sanitized_program_parses_loads_and_finishes(tmp_path, rasters):
    d, f = rasters
    cc = shutil.which("gcc") or shutil.which("cc")
    exe = str(tmp_path / "rains_san")
    sources = sorted(s for s in glob.glob(os.path.join(ROOT, "gcn10_amd", "csrc", "host", "*.c"))
                     if os.path.basename(s) != "main.c")
    # both runtimes linked statically: the program then runs in any environment, whatever else is loaded before it
    cmd = [cc, "-std=c99", "-D_GNU_SOURCE", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-pthread",
           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "rains_san_main.c")] + sources + \
          ["-lm", "-lz", "-ldl"]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(*args, status=(0,)):
        p = subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=120)
        assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
        assert p.returncode in status, (args, p.returncode, p.stdout[-2000:], p.stderr[-3000:])
        return p.stdout.split("\n")[:-1]

    # hostile texts: none but colons, a thousand members, a name of 50 000 bytes, every prefix of a good text
    long_name = "n" * 50000
    good = "a.tif:/b/c.tif:d"
    hostile = REFUSED + [":" * 300, "a:" * 1000, "a:" * 8, ("a:" * 8)[:-1], long_name, long_name + ":" + long_name,
                         long_name + ":"] + [good[:n] for n in range(len(good) + 1)]
    lines = run("parse", *hostile, status=(1,))
    assert len(lines) == len(hostile)
    for text, line in zip(hostile, lines):
        try:
            names = host.parse_rains(text)
        except host.HostError:
            assert line == "bad", text[:60]
            continue
        assert line == "%d" % len(names) + "".join(" [%s]" % n for n in names), text[:60]
    assert lines[:len(REFUSED)] == ["bad"] * len(REFUSED) and sum(ln != "bad" for ln in lines) > 8
    for text, names in GOOD:
        assert run("parse", text) == ["%d" % len(names) + "".join(" [%s]" % n for n in names)]

    # K rasters, then the refusals: nothing stays allocated (the leak check), every pointer is NULL again
    order = [2, 0, 1, 0, 2, 2, 1, 0]
    lines = run("load", GRID_TEXT, ":".join("%s/r%d.tif" % (d, j + 1) for j in order))
    assert lines == ["%d %d %d %d" % (i + 1, int(f[j].sum()), f[j][0, 0], f[j][-1, -1]) for i, j in enumerate(order)]
    assert run("load", GRID_TEXT, d + "/r2.tif") == ["1 %d %d %d" % (int(f[1].sum()), f[1][0, 0], f[1][-1, -1])]
    lines = run("load", GRID_TEXT, "%s/r1.tif:%s/r2.tif:%s/small.tif:%s/r3.tif" % (d, d, d, d), status=(1,))
    assert lines == ["error -2 rains: '%s/small.tif' has 29 x 22 pixels, the grid has 30 x 22 cells" % d]
    lines = run("load", GRID_TEXT, "%s/off.tif" % d, status=(1,))
    assert len(lines) == 1 and lines[0].startswith("error -3 rains: '%s/off.tif' does not lie on the grid" % d)
    lines = run("load", GRID_TEXT, "%s/r1.tif:%s/none.tif" % (d, d), status=(1,))
    assert len(lines) == 1 and lines[0].startswith("error -1 rains: cannot read '%s/none.tif': " % d)

    # the per-layer finish of shared cells against the plain restatement
    assert run("cells", "20000") == ["cells ok"]
