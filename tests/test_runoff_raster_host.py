"""CPU: the host side of the runoff rasters -- gcn10_runoff_bytes against a model in Python integers over all 65 536
entries, the unit that never saturates, the parser of the output unit, and the default unit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from gcn10_amd import host
from tests import runoffutil as ru
from tests.conftest import ROOT

UNITS = [1, 13, 100, 250, 65000]


def model_bytes(q, u):
    """uint8[256][256]: t[b][255] = 255; for v < 255, min(254, (2 q[b][v] + u) // (2 u)) -- Python integers only"""
    t = np.zeros((256, 256), np.uint8)
    for b in range(256):
        for v in range(255):
            t[b, v] = min(254, (2 * int(q[b][v]) + u) // (2 * u))
        t[b, 255] = 255
    return t


@pytest.fixture(scope="module")
def q_random():
    """every 16-bit value occurs, so that every unit saturates somewhere and rounds at a half somewhere"""
    q = np.random.default_rng(5).integers(0, 65536, (256, 256)).astype(np.uint16)
    q[0, :6] = (0, 1, 65535, 65534, 507, 508)
    return q


@pytest.mark.parametrize("u", UNITS)
def test_bytes_equal_the_integer_model(q_random, u):
    for q in (q_random, host.rain_tables(2.5, 0.2)):
        got = host.runoff_bytes(q, u)
        want = model_bytes(q.tolist(), u)
        np.testing.assert_array_equal(got, want)
        assert (got[:, 255] == 255).all() and (got[:, :255] <= 254).all()
    sat = host.runoff_bytes(q_random, u)
    if u < 129:                                     # 254.5 u <= 65535: the random tables hold a value that saturates
        assert (sat[:, :255] == 254).any()
    # a tie rounds up: q = (2 k + 1) u / 2 exactly, for an even u
    if u % 2 == 0:
        q = np.zeros((256, 256), np.uint16)
        q[3, 7], q[3, 8] = u // 2, u // 2 - 1           # half a count, and just below
        assert host.runoff_bytes(q, u)[3, 7:9].tolist() == [1, 0]


@pytest.mark.parametrize("unit,lam", [(1.0, 0.2), (2.5, 0.2), (0.37, 0.05), (2.54, 0.0)])
def test_the_rain_unit_as_output_unit_never_saturates_below_table_255(unit, lam):
    q = host.rain_tables(unit, lam)
    for b in range(256):
        np.testing.assert_array_equal(q[b], ru.table(b * unit, lam))
    u = host.runoff_unit_of(unit)
    assert u == int(np.floor(100.0 * unit + 0.5))
    t = host.runoff_bytes(q, u)
    for b in range(255):
        assert int(t[b, :255].max()) <= b, (b, int(t[b, :255].max()))
        assert int(q[b, :255].max()) == int(q[b, 100])
    np.testing.assert_array_equal(t, model_bytes(q.tolist(), u))


GOOD = {"1": 100, "2.5": 250, "0.01": 1, "650": 65000, "+1": 100, ".5": 50, "0.005": 1, "1e1": 1000, "0.125": 13,
        "0.0149999": 1, "649.999": 65000}
BAD = ["", " 1", "1 ", "x", "1,2", "0", "0.0049", "-1", "650.01", "651", "nan", "inf", "1mm", "1e9", "1:2", ","]


def test_the_unit_parser():
    for text, u in GOOD.items():
        assert host.parse_runoff_unit(text) == u, text
    for text in BAD:
        with pytest.raises(host.HostError):
            host.parse_runoff_unit(text)
    assert host.runoff_unit_of(0.001) == 1 and host.runoff_unit_of(2.55) == 255


def test_the_host_functions_as_a_sanitized_program(tmp_path):
    """tests/runoff_bytes_san_main.c with runoff.c under AddressSanitizer + UBSan: a program of its own, nothing preloaded"""
    cc = shutil.which("gcc") or shutil.which("cc")
    exe = str(tmp_path / "runoff_bytes_san")
    cmd = [cc, "-std=c99", "-D_GNU_SOURCE", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "runoff_bytes_san_main.c"),
           os.path.join(ROOT, "gcn10_amd", "csrc", "host", "runoff.c"), "-lm"]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(*args):
        p = subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=120)
        assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
        assert p.returncode in (0, 1), (args, p.returncode, p.stderr[-3000:])
        return p

    p = run()
    assert p.returncode == 0 and p.stdout == "cases ok\n", p.stdout
    for text, u in GOOD.items():
        assert run(text).stdout == "%d\n" % u, text
    for text in BAD + ["9" * 400, "0." + "0" * 400 + "1", "1e-400"]:
        p = run(text)
        assert p.returncode == 1 and p.stdout == "bad\n", text
