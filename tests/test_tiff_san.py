"""CPU: the GeoTIFF module (gcn10_amd/csrc/host/tiff_*.c) driven by a stand-alone program under AddressSanitizer +
UBSan with leak detection (tests/tiff_san_main.c): the three puts of the writer, plain and COG, finished, aborted and
finished after a refusal; the window reader and the read planner over the layouts of tests/test_tiff_pins.py with and
without an I/O pool and with and without the chunk cache; truncated and bit-flipped files."""
import os
import random
import shutil
import subprocess

import pytest

from tests import test_tiff_pins as pins, tiffutil
from tests.conftest import ROOT
from tests.test_host_fuzz import _mutate

N_FUZZ = 40         # per file


def _inputs(work):
    layouts = []
    for shape, skw in pins.SHAPES.items():
        for codec, ckw in pins.CODECS.items():
            name = "in_%s_%s.tif" % (shape, codec)
            tiffutil.write_tiff(str(work / name), pins.IMG, gt=pins.GT, **skw, **ckw)
            layouts.append("%s %d" % (name, 1 if codec == "packbits" else 0))
    (work / "layouts.txt").write_text("\n".join(layouts) + "\n")
    rnd, fuzz = random.Random(11), []
    for vi, kw in enumerate([dict(compression=5, predictor=2, tile=(4, 3)), dict(compression=8, rows_per_strip=3),
                             dict(compression=32773, bigtiff=True, tile=(16, 16))]):
        tiffutil.write_tiff(str(work / "seed.tif"), pins.IMG, gt=pins.GT, **kw)
        data = (work / "seed.tif").read_bytes()
        for k in range(N_FUZZ):
            name = "fuzz_%d_%02d.tif" % (vi, k)
            (work / name).write_bytes(bytes(_mutate(data, rnd)))
            fuzz.append(name)
    (work / "fuzz.txt").write_text("\n".join(fuzz) + "\n")
    return len(layouts), len(fuzz)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cc = shutil.which("gcc") or shutil.which("cc")
    exe = str(tmp_path_factory.mktemp("tiff_san") / "tiff_san")
    host = os.path.join(ROOT, "gcn10_amd", "csrc", "host")
    # both runtimes linked statically: the program then runs in any environment, whatever else is loaded before it
    cmd = [cc, "-std=c99", "-D_GNU_SOURCE", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "include"), "-I" + host, "-pthread", "-o", exe,
           os.path.join(ROOT, "tests", "tiff_san_main.c")] + \
          [os.path.join(host, f) for f in ("tiff_open.c", "tiff_codec.c", "tiff_cache.c", "tiff_window.c", "tiff_write.c",
                                           "pool.c")] + ["-lz", "-lm"]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    return exe


@pytest.mark.parametrize("cache_mb", [None, "0"], ids=["cache", "no_cache"])
def test_sanitized_tiff_module_writes_reads_and_plans(tmp_path, program, cache_mb):
    """2 x 3 puts x (2 files written and read back, one aborted, one finished with a tile missing, one finished after a
    put of a tile outside the grid) = 30 writer cases, one case per layout, one per damaged file.  The program checks
    the pixels; here: that it said so, and no sanitizer spoke.  Once with GCN10_CHUNK_CACHE_MB=0: every compressed
    chunk is then decoded into the reader's own buffers."""
    n_layouts, n_fuzz = _inputs(tmp_path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("GCN10_CHUNK_CACHE_MB", None)
    if cache_mb is not None:
        env["GCN10_CHUNK_CACHE_MB"] = cache_mb
    p = subprocess.run([program, str(tmp_path)], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert p.stdout.strip() == "tiff_san: %d cases ok" % (30 + n_layouts + n_fuzz), p.stdout[-500:]
