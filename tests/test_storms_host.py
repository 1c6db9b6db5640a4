"""CPU: several design storms on the host (csrc/host/runoff.c: gcn10_parse_storms; the config key "storms"): good texts
with and without a ratio, 1 to 8 depths, every refusal, the same texts through the config key, and the parser as a
program of its own under AddressSanitizer + UBSan.  Then the expected-value helper of the GPU tests
(tests/stormutil.py::add_words) against runoffutil.add_triples, table by table."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from gcn10_amd import host
from tests import runoffutil as ru
from tests import stormutil as su
from tests.conftest import ROOT
from tests.test_gpu_grid import maps

BAD = ("bad value for storms: '%s' (P1[:P2...][,lambda]: 1 to 8 rising depths, 0 < P <= 650 mm, 0 <= lambda < 1)")
GOOD = [("50", ([50.0], 0.2)), ("25:50:100", ([25.0, 50.0, 100.0], 0.2)), ("25.4:50.8,0.05", ([25.4, 50.8], 0.05)),
        ("1:2:3:4:5:6:7:8", ([float(v) for v in range(1, 9)], 0.2)), ("1:2:3:4:5:6:7:650,0", ([1.0, 2, 3, 4, 5, 6, 7, 650], 0.0)),
        ("1e-3:+7.5:0x10,.999", ([0.001, 7.5, 16.0], 0.999)), ("50:50.01", ([50.0, 50.01], 0.2)),
        ("0.004:0.006", ([0.004, 0.006], 0.2))]                 # N = 0 and 1: they rise in hundredths
REFUSED = ["", " ", "1:2:3:4:5:6:7:8:9",                        # none, nine depths
           "50.001:50.004", "50:50", "0.001:0.004",             # equal N
           "50:25", "25:100:50",                                # falling depths
           "25::50", ":25", "25:", "25:50:", "25:50,", ",0.2", "25,,0.2",       # an empty field, a trailing ':'
           "50x", "25:50x", "25:50 ", " 25:50", "25: 50", "25:50,0.2x", "25 :50",      # text behind or before a value
           "nan", "25:nan", "inf", "25:inf", "25,nan", "1e999", "25:1e999",
           "0", "25:0", "-1:25", "650.01", "25:650.01",         # a depth out of range
           "25:50,1", "25:50,-0.1", "25,1.5",                   # a ratio out of range
           "25,0.2,0.3", "25,0.2:50", "25;50", "P"]
BASE = "hysogs_data_path=h\nesa_data_path=e\nblocks_shp_path=b\nlookup_table_path=l\nlog_dir=d\n"


@pytest.mark.parametrize("text,want", GOOD)
def test_the_parser_reads_depths_and_a_ratio(text, want):
    assert host.parse_storms(text) == want
    N = [int(host.runoff_table(p, want[1])[100]) for p in want[0]]
    assert all(b > a for a, b in zip(N, N[1:]))
    if len(want[0]) == 1:       # one depth: the text and the values of the storm key
        assert host.parse_storm(text) == (want[0][0], want[1])


@pytest.mark.parametrize("text", REFUSED)
def test_the_parser_refuses(text, tmp_path):
    with pytest.raises(host.HostError) as e:
        host.parse_storms(text)
    assert str(e.value) == BAD % text
    # the config key refuses the same texts, in the parser's words (a value is trimmed before it is read, so white
    # space around a good value is no error there)
    if text.strip() in ("25:50",):
        return
    (tmp_path / "c.txt").write_text(BASE + "storms=%s\n" % text)
    with pytest.raises(host.HostError) as e:
        host.parse_config(str(tmp_path / "c.txt"))
    assert str(e.value) == BAD % text.strip()


def test_the_equal_names_are_equal_in_hundredths():
    """What the refusal of 50.001:50.004 rests on: both are N = 5000."""
    for a, b in ((50.001, 50.004), (0.001, 0.004)):
        assert int(host.runoff_table(a)[100]) == int(host.runoff_table(b)[100])


@pytest.mark.parametrize("text,want", GOOD)
def test_the_config_key(tmp_path, text, want):
    (tmp_path / "c.txt").write_text(BASE + "storms = %s \n" % text)
    cfg = host.parse_config(str(tmp_path / "c.txt"))
    assert cfg["storms"] == text and cfg["n_storms"] == len(want[0]) and cfg["storms_lambda"] == want[1]
    assert cfg["storms_p"][:len(want[0])] == want[0]
    assert cfg["storm"] is None
    (tmp_path / "c.txt").write_text(BASE + "storm=50\n")
    cfg = host.parse_config(str(tmp_path / "c.txt"))
    assert cfg["storms"] is None and cfg["n_storms"] == 0 and cfg["storm"] == "50"


def test_the_parser_as_a_sanitized_program(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    exe = str(tmp_path / "storms_san")
    # both runtimes linked statically: the program then runs in any environment, whatever else is loaded before it
    cmd = [cc, "-std=c99", "-D_GNU_SOURCE", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "storms_san_main.c"),
           os.path.join(ROOT, "gcn10_amd", "csrc", "host", "runoff.c"), "-lm"]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(*args):
        p = subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=120)
        assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
        assert p.returncode in (0, 1), (args, p.returncode, p.stderr[-3000:])
        return p

    # long and truncated lists: many depths, a long number, every prefix of a good text
    long_lists = [":".join(str(v) for v in range(1, n + 1)) for n in (9, 10, 64, 400)]
    long_lists += ["9" * 400, "1:" + "5" + "0" * 400, "1:2," + "0" * 300 + ".5", ":" * 300, "1:" * 300, "1," * 300]
    good = "1.5:25:50.25:100:200:300:400:650,0.05"
    prefixes = [good[:n] for n in range(len(good) + 1)]
    p = run(*(REFUSED + long_lists))
    lines = p.stdout.split("\n")[:-1]
    assert p.returncode == 1 and len(lines) == len(REFUSED) + len(long_lists)
    for text, line in zip(REFUSED + long_lists, lines):
        assert (line == "bad") == (text != "1:2," + "0" * 300 + ".5"), text
    p = run(*prefixes)
    lines = p.stdout.split("\n")[:-1]
    assert len(lines) == len(prefixes)
    for text, line in zip(prefixes, lines):
        try:
            P, lam = host.parse_storms(text)
        except host.HostError:
            assert line == "bad", text
            continue
        N = [int(ru.table(v, lam)[100]) for v in P]
        assert line == "storms %d %.17g %s | %s" % (len(P), lam, " ".join("%.17g" % v for v in P),
                                                    " ".join(str(n) for n in N)), text
    assert lines[-1].endswith(" | 150 2500 5025 10000 20000 30000 40000 65000") and lines[0] == "bad" and "bad" in lines[1:] and \
        sum(ln != "bad" for ln in lines) > 8
    for text, want in GOOD:
        p = run(text)
        assert p.returncode == 0 and p.stdout.startswith("storms %d %.17g " % (len(want[0]), want[1])), p.stdout


def test_add_words_adds_what_add_triples_adds():
    """tests/stormutil.py::add_words, table by table, against runoffutil.add_triples (np.add.at at this size)."""
    rng = np.random.default_rng(2)
    W, rows = 333, 77
    raster = rng.choice(np.array([0, 1, 77, 100, 254, 255], np.uint8), size=(rows, W))
    cellx, celly = maps(W, rows, 8.5, 17.3, (2, 1), (1, 2))
    ws = su.table_set(8, 0)
    assert sorted(su.table_names(8, 0)[:7]) == sorted(su.ORDER)
    got = np.zeros((int(celly.max()) + 1, int(cellx.max()) + 1, 10), np.int64)
    su.add_words(got, raster, cellx, celly, ws)
    for j in range(8):
        want = np.zeros(got.shape[:2] + (3,), np.int64)
        ru.add_triples(want, raster, cellx, celly, ws[j])
        np.testing.assert_array_equal(got[..., [0, 1, 2 + j]], want)
    assert got[..., 1].max() > 0 and (raster == 255).any()
    su.add_words(got, raster, cellx, celly, ws)                # it ADDS
    np.testing.assert_array_equal(got[..., [0, 1, 9]], 2 * want)
    np.testing.assert_array_equal(su.cn_arrays(got, ws)[3], ru.cn_array(got[..., [0, 1, 5]], ws[3]))
