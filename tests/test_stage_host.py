"""CPU: the chunk stager that the input side and the verifier share (gcn10_amd/csrc/host/stage.c), driven by a
stand-alone program under AddressSanitizer + UBSan (tests/stage_san_main.c).  The product's staging buffers are 64 MiB,
so no run of the program at test size reaches the stager's edges; here the ring is 2 buffers of 4 KiB."""
import os
import shutil
import subprocess

from tests.conftest import ROOT


def test_sanitized_stager_stages_every_chunk_with_and_without_a_pool(tmp_path):
    """Chunk counts 0, 1, one buffer full, one byte more, 100 of mixed sizes; a slot of exactly one buffer; a chunk one
    byte larger (bad == 2); chunks beyond the end of the file and on a closed descriptor (bad == 1, zeros staged); the
    ring growing between two calls.  The program checks that every good chunk's bytes lie at d_comp + in_off with 16
    zero bytes behind them and that bad[] is exactly the expected set; here: that it said so, and no sanitizer spoke."""
    cc = shutil.which("gcc") or shutil.which("cc")
    exe = str(tmp_path / "stage_san")
    host = os.path.join(ROOT, "gcn10_amd", "csrc", "host")
    # both runtimes linked statically: the program then runs in any environment, whatever else is loaded before it
    cmd = [cc, "-std=c99", "-D_GNU_SOURCE", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-static-libasan", "-static-libubsan",
           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-I" + host, "-pthread",
           "-o", exe, os.path.join(ROOT, "tests", "stage_san_main.c"),
           os.path.join(host, "stage.c"), os.path.join(host, "pool.c")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    work = tmp_path / "work"
    work.mkdir()
    p = subprocess.run([exe, str(work)], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    # the job list, and 11 cases of the stager without and 11 with a pool
    assert p.stdout.strip() == "stage_san: 23 cases ok", p.stdout[-500:]
