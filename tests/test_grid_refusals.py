"""CPU: every way a grid run (config key grid, --grid) stops before a GPU is opened: exit status 1, the exact text on
stderr, nothing created.  Run the way tests/test_run_refusals.py runs its own table, which stays the list of the other
modes; then the start-up failure with a GPU library that lacks the grid entry points (the stub of tests/stub_gpu)."""
import os
import subprocess

import numpy as np
import pytest

from tests import tiffutil, zoneutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQUARE = [[(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]]
LAUNCHER_VARS = ("OMPI_COMM_WORLD_RANK", "OMPI_COMM_WORLD_SIZE", "PMI_RANK", "PMI_SIZE", "PMIX_RANK", "PMIX_SIZE",
                 "SLURM_PROCID", "SLURM_NTASKS")
PX = 8.3333333333330430e-05
GRID = "9.9995,50.0005,0.0021,0.0021,30,22"
BAD = "(xmin,ymax,dx,dy,nx,ny)"


def _config(tmp_path, **extra):
    p = tmp_path / "cfg.txt"
    keys = dict(hysogs_data_path="h", esa_data_path="e", blocks_shp_path="b", lookup_table_path="l",
                log_dir=str(tmp_path / "logs"))
    keys.update(extra)
    p.write_text("".join("%s=%s\n" % kv for kv in keys.items() if kv[1] is not None))
    return str(p)


def _gcn10(args, cwd, env=None):
    e = {k: v for k, v in os.environ.items() if k not in LAUNCHER_VARS}
    e.update(env or {})
    return subprocess.run([os.path.join(ROOT, "bin", "gcn10")] + args, cwd=str(cwd), capture_output=True, text=True,
                          timeout=120, env=e)


@pytest.fixture()
def zones(tmp_path):
    zoneutil.write_zone_shapefile(str(tmp_path / "zones"), [(1, SQUARE)])
    return str(tmp_path / "zones.shp")


@pytest.fixture()
def esa(tmp_path):
    """A landcover file at the real pixel size: the cell size is checked against it."""
    tiffutil.write_tiff(str(tmp_path / "esa.tif"), np.full((40, 60), 10, np.uint8), gt=[10.0, PX, 0.0, 50.0, 0.0, -PX],
                        compression=8, tile=(256, 256))
    return str(tmp_path / "esa.tif")


# name -> (config keys, arguments behind "-c <config>", environment, stderr); "{zones}" and "{esa}" stand for the files
# above; a message without "[rank 0] " comes from the config parser, as it words it
REFUSALS = {
    "bad --grid: a field is missing": ({}, ["--grid", "1,2,3,4,5"], {}, "[rank 0] bad value for grid: '1,2,3,4,5' " + BAD + "\n"),
    "bad --grid: text behind it": ({}, ["--grid", GRID + "x"], {}, "[rank 0] bad value for grid: '" + GRID + "x' " + BAD + "\n"),
    "bad --grid: dx = 0": ({}, ["--grid", "1,2,0,4,5,6"], {}, "[rank 0] bad value for grid: '1,2,0,4,5,6' " + BAD + "\n"),
    "bad --grid: more than 2^26 cells": ({}, ["--grid", "1,2,3,4,5,13421773"], {},
                                         "[rank 0] bad value for grid: '1,2,3,4,5,13421773' " + BAD + "\n"),
    "bad --grid over a good key": (dict(grid=GRID), ["--grid", "nan,2,3,4,5,6"], {},
                                   "[rank 0] bad value for grid: 'nan,2,3,4,5,6' " + BAD + "\n"),
    "bad grid key": (dict(grid="1,2,3,4,-5,6"), [], {}, "bad value for grid: '1,2,3,4,-5,6' " + BAD + "\n"),
    "bad grid key: more than 2^26 cells": (dict(grid="1,2,3,4,8193,8192"), [], {},
                                           "bad value for grid: '1,2,3,4,8193,8192' " + BAD + "\n"),
    "cells under 8 pixels wide": (dict(esa_data_path="{esa}"), ["--grid", "10,50,0.00066,0.0021,30,22"], {},
                                  "[rank 0] bad value for grid: '10,50,0.00066,0.0021,30,22' (cells under 8 landcover "
                                  "pixels of 8.333333333333043e-05 x 8.333333333333043e-05)\n"),
    "cells under 8 pixels high": (dict(esa_data_path="{esa}", grid="10,50,0.0021,0.00066,30,22"), [], {},
                                  "[rank 0] bad value for grid: '10,50,0.0021,0.00066,30,22' (cells under 8 landcover "
                                  "pixels of 8.333333333333043e-05 x 8.333333333333043e-05)\n"),
    "grid with --zonal": ({}, ["--zones", "{zones}", "--grid", GRID], {}, "[rank 0] grid cannot be combined with --zonal\n"),
    "grid key with zonal=1": (dict(grid=GRID, zonal=1, zones_shp_path="{zones}"), [], {},
                              "[rank 0] grid cannot be combined with --zonal\n"),
    "grid with --verify": ({}, ["--grid", GRID, "--verify"], {},
                           "[rank 0] grid cannot be combined with --verify (the grid rasters are not verified)\n"),
    "grid with --aggregate": ({}, ["--grid", GRID, "--aggregate", "25"], {},
                              "[rank 0] grid cannot be combined with aggregate\n"),
    "grid with aggregate=7": (dict(aggregate=7), ["--grid", GRID], {}, "[rank 0] grid cannot be combined with aggregate\n"),
    "grid with --overwrite": ({}, ["--grid", GRID, "-o"], {},
                              "[rank 0] grid writes one raster per lookup and condition and cannot be combined with "
                              "--overwrite\n"),
    "grid under a launcher": ({}, ["--grid", GRID], {"OMPI_COMM_WORLD_RANK": "1", "OMPI_COMM_WORLD_SIZE": "2"},
                              "[rank 0] grid runs as one process: merging rasters across launcher ranks is not "
                              "supported\n"),
    "grid with --compress lzw": ({}, ["--grid", GRID, "--compress", "lzw"], {},
                                 "[rank 0] bad value for compress: 'lzw' with grid (the grid rasters are encoded on the "
                                 "host; there is no host LZW encoder)\n"),
    "grid key with compress=lzw": (dict(grid=GRID, compress="lzw"), [], {},
                                   "[rank 0] bad value for compress: 'lzw' with grid (the grid rasters are encoded on the "
                                   "host; there is no host LZW encoder)\n"),
}


def _nothing_written(tmp_path):
    return not (tmp_path / "logs").exists() and not [f for f in os.listdir(tmp_path) if f.startswith("cn_")]


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refused_before_any_gpu(tmp_path, zones, esa, case):
    keys, args, env, stderr = REFUSALS[case]
    fill = dict(zones=zones, esa=esa, tmp=str(tmp_path))
    args = [a.format(**fill) for a in args]
    keys = {k: v.format(**fill) if isinstance(v, str) else v for k, v in keys.items()}
    p = _gcn10(["-c", _config(tmp_path, **keys)] + args, tmp_path, env)
    assert p.returncode == 1, p.stdout + p.stderr
    assert p.stderr == stderr
    assert p.stdout == ""
    assert _nothing_written(tmp_path)


def test_cells_of_exactly_8_pixels_are_not_refused_for_their_size(tmp_path, esa):
    """8 pixels pass the size check: the run goes on to the GPU library (here: one that cannot be loaded)."""
    text = "10,50,%r,%r,3,3" % (8 * PX, 8 * PX)
    p = _gcn10(["-c", _config(tmp_path, esa_data_path=esa), "--grid", text], tmp_path,
               {"GCN10_GPU_LIB": str(tmp_path / "nothing.so")})
    assert p.returncode == 1 and "bad value for grid" not in p.stderr and "cannot load" in p.stderr, p.stderr


# ---- a GPU library without the entry points: the stub has neither ------------------------------------------------

@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("stub") / "libstub_gpu.so")
    subprocess.run(["gcc", "-std=c11", "-O1", "-fPIC", "-shared", "-pthread", "-I" + os.path.join(ROOT, "include"),
                    "-o", so, os.path.join(ROOT, "tests", "stub_gpu", "stub_gpu.c"), "-lz"], check=True)
    return so


@pytest.mark.parametrize("how", ["flag", "key", "with cog and stats"])
def test_a_gpu_library_without_the_entry_points_fails_at_start(tmp_path, stub, how):
    keys = dict(grid=GRID) if how == "key" else {}
    args = [] if how == "key" else ["--grid", GRID] + (["--cog", "--stats"] if how == "with cog and stats" else [])
    p = _gcn10(["-c", _config(tmp_path, **keys)] + args, tmp_path, {"GCN10_GPU_LIB": stub})
    assert p.returncode == 1, p.stdout + p.stderr
    assert p.stderr == "[rank 0] %s lacks gcn10_gpu_grid_sums (needed by grid=%s)\n" % (stub, GRID)
    assert p.stdout == ""
    assert _nothing_written(tmp_path)
