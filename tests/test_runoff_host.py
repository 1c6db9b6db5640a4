"""CPU: the design storm of the runoff-weighted composites on the host (csrc/host/runoff.c): the runoff table against
the numpy float64 restatement of its lines (tests/runoffutil.py), every refusal of the parser, the cell rule on hand-made
triples, and the three of them as a program of their own under AddressSanitizer + UBSan."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from gcn10_amd import host
from tests import runoffutil as ru
from tests.conftest import ROOT

DEPTHS = [0.5, 1, 25.4, 50, 100, 650]
RATIOS = [0, 0.05, 0.2]
REFUSED = ["", " ", "50x", "50 ", " 50", "0", "0.0", "650.01", "nan", "inf", "-1", "50,1", "50,-0.1", "50,nan",
           "50,0.2,0.3", "50,", ",0.2", "50;0.2", "1e999", "P"]
BAD = "bad value for storm: '%s' (P[,lambda]: 0 < P <= 650 mm, 0 <= lambda < 1)"


@pytest.mark.parametrize("lam", RATIOS)
@pytest.mark.parametrize("P", DEPTHS)
def test_the_table_equals_the_numpy_restatement(P, lam):
    q = host.runoff_table(P, lam)
    want = ru.table(P, lam)
    np.testing.assert_array_equal(q, want)
    assert q.dtype == np.uint16 and q.shape == (256,)
    assert (np.diff(q[:101].astype(np.int64)) >= 0).all()           # never decreases over 0..100
    assert q[0] == 0 and q[255] == 0
    assert (q[101:255] == q[100]).all() and int(q[100]) == int(np.floor(100.0 * P + 0.5))


def test_the_table_of_50_mm_has_no_plateau_above_its_threshold():
    """What the uniform-cell test below relies on."""
    q = host.runoff_table(50, 0.2).astype(np.int64)
    t = ru.threshold(q)
    assert 1 < t < 100 and (q[:t] == 0).all() and (np.diff(q[t - 1:101]) > 0).all()


@pytest.mark.parametrize("text,want", [("50", (50.0, 0.2)), ("25.4,0.05", (25.4, 0.05)), ("650", (650.0, 0.2)),
                                       ("1e-3,0", (0.001, 0.0)), ("+7.5,.999", (7.5, 0.999)), ("0x10", (16.0, 0.2))])
def test_the_parser_reads_a_depth_and_a_ratio(text, want):
    assert host.parse_storm(text) == want


@pytest.mark.parametrize("text", REFUSED)
def test_the_parser_refuses(text, tmp_path):
    with pytest.raises(host.HostError) as e:
        host.parse_storm(text)
    assert str(e.value) == BAD % text
    # the config key refuses the same texts, in the parser's words (a value is trimmed before it is read, so white
    # space around a good value is no error there)
    if text.strip() == "50":
        return
    (tmp_path / "c.txt").write_text("hysogs_data_path=h\nesa_data_path=e\nblocks_shp_path=b\nlookup_table_path=l\n"
                                    "log_dir=d\nstorm=%s\n" % text)
    with pytest.raises(host.HostError) as e:
        host.parse_config(str(tmp_path / "c.txt"))
    assert str(e.value) == BAD % text.strip()


def test_the_config_key(tmp_path):
    base = "hysogs_data_path=h\nesa_data_path=e\nblocks_shp_path=b\nlookup_table_path=l\nlog_dir=d\n"
    (tmp_path / "c.txt").write_text(base + "storm = 25.4,0.05 \n")
    cfg = host.parse_config(str(tmp_path / "c.txt"))
    assert (cfg["storm"], cfg["storm_p"], cfg["storm_lambda"]) == ("25.4,0.05", 25.4, 0.05)
    (tmp_path / "c.txt").write_text(base)
    cfg = host.parse_config(str(tmp_path / "c.txt"))
    assert cfg["storm"] is None and cfg["grid"] is None


def hand_made_triples(q):
    """(s, n, sw) that meet every branch of the cell rule for the table q of P = 50, lambda = 0.2."""
    q = [int(v) for v in q]
    t = ru.threshold(q)
    out = [(0, 0, 0), (17, 0, 5),                               # n = 0
           (5, 2, 0), (7, 2, 0), (1, 3, 0), (254 << 31, 1 << 31, 0)]   # sw = 0: the mean byte, exact halves round up
    out += [(c * 7, 7, q[c] * 7) for c in range(t, 101)]        # a uniform cell of every c from the threshold to 100
    for c in (t, t + 1, 60, 99, 100):                           # n q[c] == sw exactly, and one beside it
        n = 12345
        out += [(c * n, n, n * q[c]), (c * n, n, n * q[c] + 1), (c * n, n, n * q[c] - 1)]
    out += [(100 * 3, 3, 3 * q[100]), (1, 1, 1), (3, 9, 1)]     # sw = n q[100]; the smallest sums
    big = 1 << 40
    out += [(70 * big, big, big * q[70]), (70 * big, big, big * q[70] + 1), (70 * big, big, big * q[100]),
            (70 * big, big, 0), (70 * big, big, 1)]             # n = 2^40
    return out


def test_the_cell_rule_on_hand_made_triples():
    q = host.runoff_table(50, 0.2)
    t = ru.threshold(q)
    triples = hand_made_triples(q)
    for s, n, sw in triples:
        assert host.runoff_cn(s, n, sw, q) == ru.cn(s, n, sw, q), (s, n, sw)
    got = {tr: host.runoff_cn(*tr, q) for tr in triples}
    assert got[(0, 0, 0)] == 255 and got[(17, 0, 5)] == 255
    assert got[(5, 2, 0)] == 3 and got[(7, 2, 0)] == 4 and got[(1, 3, 0)] == 0 and got[(254 << 31, 1 << 31, 0)] == 254
    for c in range(t, 101):
        assert got[(c * 7, 7, int(q[c]) * 7)] == c              # a cell of one CN gets that CN back
    n = 12345
    assert got[(60 * n, n, n * int(q[60]))] == 60 and got[(60 * n, n, n * int(q[60]) + 1)] == 61
    assert got[(60 * n, n, n * int(q[60]) - 1)] == 60
    assert got[(100 * n, n, n * int(q[100]) + 1)] == 100        # beyond the table's maximum: 100, never past the table
    assert got[(1, 1, 1)] == t and got[(70 << 40, 1 << 40, 1)] == t and got[(70 << 40, 1 << 40, 0)] == 70
    assert got[(70 << 40, 1 << 40, (1 << 40) * int(q[70]) + 1)] == 71
    # the vectorised statement the GPU tests use agrees with the scalar one
    small = np.array([tr for tr in triples if tr[1] < (1 << 46)], np.int64)
    np.testing.assert_array_equal(ru.cn_array(small, q), [ru.cn(*tr, q) for tr in small.tolist()])


def test_the_host_functions_as_a_sanitized_program(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    exe = str(tmp_path / "runoff_san")
    # both runtimes linked statically: the program then runs in any environment, whatever else is loaded before it
    cmd = [cc, "-std=c99", "-D_GNU_SOURCE", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "runoff_san_main.c"),
           os.path.join(ROOT, "gcn10_amd", "csrc", "host", "runoff.c"), "-lm"]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(*args):
        p = subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=120)
        assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
        assert p.returncode in (0, 1), (args, p.returncode, p.stderr[-3000:])
        return p

    for text in REFUSED + ["9" * 400, "5" + "0" * 400, "1," + "0" * 300 + ".5", "-", "+", ".", "1e", "0x", ",", ",,"]:
        p = run(text)
        if p.returncode == 1:
            assert p.stdout == "bad\n", text
        else:
            assert text in ("1," + "0" * 300 + ".5",), text
    triples = hand_made_triples(host.runoff_table(50, 0.2)) + [(2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1),
                                                                (0, 2 ** 63, 2 ** 64 - 1), (0, 1, 2 ** 64 - 1)]
    for P in DEPTHS:
        for lam in RATIOS:
            args = ["%r,%r" % (float(P), float(lam))]
            if (P, lam) == (50, 0.2):
                args += [str(v) for tr in triples for v in tr]
            p = run(*args)
            lines = p.stdout.split("\n")
            assert p.returncode == 0 and lines[0] == "storm %.17g %.17g" % (P, lam), p.stdout[:200]
            assert [int(v) for v in lines[1].split()] == ru.table(P, lam).tolist()
            if (P, lam) == (50, 0.2):
                q = ru.table(P, lam)
                # the last three wrap in 64 bits by design of the type; the rule is stated for sums that fit
                assert lines[2:2 + len(triples) - 3] == ["cn %d" % ru.cn(*tr, q) for tr in triples[:-3]]
                assert len(lines) == 2 + len(triples) + 1
