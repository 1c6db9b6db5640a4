"""CPU: the shape of what a run says -- the console and rank_0.log of bin/gcn10 over two tiny blocks with one worker,
against the stub of tests/stub_gpu, in both sink modes (gpu_deflate=1: gate, append and finish jobs; gpu_deflate=0:
host deflate and finish jobs).  Every number becomes N and every absolute path P; what is left -- which lines, in which
order, with which words -- is compared with tests/golden/run_log_shape.txt, recorded from the program as it was before
the run driver was split into steps.

A block is 300 x 300 px and a strip 256 rows: two strips, the second ragged, over a 2 x 2 tile grid."""
import os
import re
import subprocess

import numpy as np
import pytest
from PIL import Image

from tests import tiffutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "run_log_shape.txt")
PX = 1.0 / 1024                     # a power of two: the blocks' edges fall on pixel edges exactly
ESA_GT = [10.0, PX, 0.0, 50.0, 0.0, -PX]
SOIL_GT = [10.0 - 12.5 * PX, 25 * PX, 0.0, 50.0 + 12.5 * PX, 0.0, -25 * PX]
MODES = ("gpu_deflate=1", "gpu_deflate=0")
LAUNCHER_VARS = ("OMPI_COMM_WORLD_RANK", "OMPI_COMM_WORLD_SIZE", "PMI_RANK", "PMI_SIZE", "PMIX_RANK", "PMIX_SIZE",
                 "SLURM_PROCID", "SLURM_NTASKS")


def normalise(text):
    """Absolute paths -> P, then numbers -> N.  A number takes its sign along: the NUMA node of the stub's PCI address
    is -1 on one machine and 0 on the next."""
    text = re.sub(r"(?<![\w.])/[^\s]+", "P", text)
    return re.sub(r"-?[0-9][0-9.]*", "N", text)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("log_shape"))
    stub = os.path.join(tmp, "libstub_gpu.so")
    subprocess.run(["gcc", "-std=c11", "-O1", "-fPIC", "-shared", "-pthread", "-I" + os.path.join(ROOT, "include"),
                    "-o", stub, os.path.join(ROOT, "tests", "stub_gpu", "stub_gpu.c"), "-lz"], check=True)
    rng = np.random.default_rng(5)
    H, W = 300, 600
    esa = np.repeat(np.repeat(rng.choice(np.array([10, 20, 30, 40, 50, 60, 80, 90], np.uint8), size=(H // 20, W // 20)),
                              20, axis=0), 20, axis=1)
    soil = rng.choice(np.array([1, 2, 3, 4, 11, 12, 13, 14], np.uint8), size=(H // 25 + 2, W // 25 + 2))
    tiffutil.write_tiff(os.path.join(tmp, "esa.tif"), esa, gt=ESA_GT, compression=8, tile=(256, 256))
    tiffutil.write_tiff(os.path.join(tmp, "soil.tif"), soil, gt=SOIL_GT, compression=5, rows_per_strip=8)
    tiffutil.write_block_shapefile(os.path.join(tmp, "blocks"),
                                   [(201 + i, 10.0 + 300 * PX * i, 50.0 - 300 * PX, 10.0 + 300 * PX * (i + 1), 50.0)
                                    for i in range(2)])
    return tmp, stub


def _run(world, mode):
    tmp, stub = world
    work = os.path.join(tmp, "run_" + mode.replace("=", "_"))
    os.makedirs(work)
    with open(os.path.join(work, "config.txt"), "w") as f:
        f.write("hysogs_data_path=%s\nesa_data_path=%s\nblocks_shp_path=%s\nlookup_table_path=%s\nlog_dir=%s\n"
                "strip_rows=256\nio_threads=2\nworkers_per_gpu=1\n%s\n"
                % (os.path.join(tmp, "soil.tif"), os.path.join(tmp, "esa.tif"), os.path.join(tmp, "blocks.shp"),
                   os.path.join(ROOT, "tests", "golden", "lookups"), os.path.join(work, "logs"), mode))
    env = {k: v for k, v in os.environ.items() if k not in LAUNCHER_VARS and not k.startswith("GCN10_")}
    env.update(GCN10_GPU_LIB=stub, GCN10_OVERSUBSCRIBE="1", GCN10_NO_NUMA_BIND="1")
    p = subprocess.run([os.path.join(ROOT, "bin", "gcn10"), "-c", "config.txt", "--gpus", "1"], cwd=work,
                       capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert sorted(os.listdir(os.path.join(work, "logs"))) == ["rank_0.log"]
    for bid in (201, 202):          # the blocks are what the fixture's shape stands for
        assert Image.open(os.path.join(work, "cn_rasters_drained", "cn_g_ii_%d.tif" % bid)).size == (300, 300)
    with open(os.path.join(work, "logs", "rank_0.log")) as f:
        log = f.read()
    # the sink path of the mode ran: jobs of its kinds, none of the other's.  (2 blocks x 2 strips x 18 rasters are 72
    # appends or host deflates, 4 gates and 36 files; a pool thread books a job after it has reported it done, so the
    # line may miss the last ones.)
    m = re.search(r"by job: appending a raster's strip \S+ \((\d+)\), waiting for a strip's bytes \S+ \((\d+)\), "
                  r"finishing files \S+ \((\d+)\), host deflate \S+ \((\d+)\)", log)
    assert m, log
    n_put, n_gate, n_finish, n_row = (int(n) for n in m.groups())
    assert 0 < n_finish <= 36
    if mode == "gpu_deflate=1":
        assert 0 < n_put <= 72 and 0 < n_gate <= 4 and n_row == 0
    else:
        assert n_put == 0 and n_gate == 0 and 0 < n_row <= 72
    return "== %s: console ==\n%s== %s: rank_0.log ==\n%s" % (mode, normalise(p.stdout + p.stderr), mode, normalise(log))


def shape(world):
    return "".join(_run(world, mode) for mode in MODES)


def test_console_and_log_keep_their_shape(world):
    got = shape(world)
    with open(GOLDEN) as f:
        want = f.read()
    assert got.splitlines() == want.splitlines()
