"""CPU: every way gcn10_run stops before a GPU is opened, in one table: exit status 1, the exact text on stderr, no
output directory.  The refusals of the command line and of the combinations of modes come first; then the start-up
failures with a GPU library that lacks an optional entry point a mode needs (the stub of tests/stub_gpu lacks all six).
Several of these also sit, with looser matches, in test_lzw_cli.py, test_stats_cli.py, test_zonal_cli.py and
test_aggregate_host.py; this table is the complete list."""
import os
import subprocess

import pytest

from tests import zoneutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQUARE = [[(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]]
LAUNCHER_VARS = ("OMPI_COMM_WORLD_RANK", "OMPI_COMM_WORLD_SIZE", "PMI_RANK", "PMI_SIZE", "PMIX_RANK", "PMIX_SIZE",
                 "SLURM_PROCID", "SLURM_NTASKS")
LZW_HOST = ("bad value for compress: 'lzw' with gpu_deflate=0 (LZW tiles are encoded on the GPU only; there is no host "
            "LZW encoder)")
COG_HOST = ("bad value for cog: '1' with gpu_deflate=0 (overviews are built and encoded on the GPU only; there is no "
            "host fallback)")


def _config(tmp_path, **extra):
    p = tmp_path / "cfg.txt"
    keys = dict(hysogs_data_path="h", esa_data_path="e", blocks_shp_path="b", lookup_table_path="l",
                log_dir=str(tmp_path / "logs"))
    keys.update(extra)
    p.write_text("".join("%s=%s\n" % kv for kv in keys.items() if kv[1] is not None))      # None: the key is left out
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


# name -> (config keys, arguments behind "-c <config>", environment, stderr).  "{zones}" stands for the zone shapefile,
# "{tmp}" for the test's directory; a message without "[rank 0] " comes from the config parser, as it words it.
REFUSALS = {
    "missing -c": (None, [], {}, "[rank 0] missing -c/--config <file>; see 'gcn10 -h' for usage.\n"),
    "unreadable config": (None, ["-c", "{tmp}/nothing.txt"], {}, "cannot open config '{tmp}/nothing.txt'\n"),
    "config without a required key": (dict(lookup_table_path=None), [], {},
                                      "missing one of: hysogs_data_path, esa_data_path,\n"
                                      "blocks_shp_path, lookup_table_path, log_dir\n"),
    "bad --lookups": ({}, ["--lookups", "q_ii"], {},
                      "[rank 0] bad --lookups / --conditions value; see 'gcn10 -h' for usage.\n"),
    "bad --conditions": ({}, ["--conditions", "damp"], {},
                         "[rank 0] bad --lookups / --conditions value; see 'gcn10 -h' for usage.\n"),
    "bad lookups key": (dict(lookups="q_ii"), [], {},
                        "bad value for lookups: 'q_ii' (names like g_ii, p_i,f_iii or all)\n"),
    "bad --compress": ({}, ["--compress", "zstd"], {}, "[rank 0] bad value for compress: 'zstd' (deflate or lzw)\n"),
    "bad compress key": (dict(compress="zstd"), [], {}, "bad value for compress: 'zstd' (deflate or lzw)\n"),
    "--compress lzw with gpu_deflate=0": (dict(gpu_deflate=0), ["--compress", "lzw"], {}, "[rank 0] " + LZW_HOST + "\n"),
    "compress=lzw with gpu_deflate=0": (dict(gpu_deflate=0, compress="lzw"), [], {}, LZW_HOST + "\n"),
    "bad --overview-resampling": ({}, ["--overview-resampling", "cubic"], {},
                                  "[rank 0] bad value for overview_resampling: 'cubic' (nearest or average)\n"),
    "bad --nodata": ({}, ["--nodata", "256"], {}, "[rank 0] bad value for nodata: '256' (none or an integer 0..255)\n"),
    "--verify --overwrite": ({}, ["--verify", "--overwrite"], {},
                             "[rank 0] --verify writes nothing and cannot be combined with --overwrite\n"),
    "verify=1 --overwrite": (dict(verify=1), ["-o"], {},
                             "[rank 0] --verify writes nothing and cannot be combined with --overwrite\n"),
    "--cog with gpu_deflate=0": (dict(gpu_deflate=0), ["--cog"], {}, "[rank 0] " + COG_HOST + "\n"),
    "cog=1 with gpu_deflate=0": (dict(gpu_deflate=0, cog=1), [], {}, COG_HOST + "\n"),
    "zonal without zones": ({}, ["--zonal"], {},
                            "[rank 0] zonal=1 needs the zone polygons: zones_shp_path=<file.shp> or --zones <file.shp>\n"),
    "zonal with --overwrite": ({}, ["--zones", "{zones}", "--overwrite"], {},
                               "[rank 0] --zonal writes no raster and cannot be combined with --overwrite\n"),
    "zonal with --verify": ({}, ["--zones", "{zones}", "--verify"], {},
                            "[rank 0] --zonal cannot be combined with --verify\n"),
    "zonal under a launcher": ({}, ["--zones", "{zones}"], {"OMPI_COMM_WORLD_RANK": "1", "OMPI_COMM_WORLD_SIZE": "2"},
                               "[rank 0] --zonal runs as one process: merging tables across launcher ranks is not "
                               "supported\n"),
    "zone file that does not open": ({}, ["--zones", "{tmp}/nothing.shp"], {},
                                     "[rank 0] cannot read the zones of {tmp}/nothing.shp: not a shapefile\n"),
    "bad --aggregate": ({}, ["--aggregate", "1"], {},
                        "[rank 0] bad value for aggregate: '1' (0 or an integer 2..256)\n"),
    "bad --aggregate behind the zones": ({}, ["--zones", "{zones}", "--aggregate", "x"], {},
                                         "[rank 0] bad value for aggregate: 'x' (0 or an integer 2..256)\n"),
    "bad aggregate key": (dict(aggregate=300), [], {}, "bad value for aggregate: '300' (0 or an integer 2..256)\n"),
    "aggregate with --zonal": (dict(aggregate=7), ["--zones", "{zones}"], {},
                               "[rank 0] aggregate cannot be combined with --zonal\n"),
    "aggregate with --verify": ({}, ["--aggregate", "25", "--verify"], {},
                                "[rank 0] aggregate cannot be combined with --verify (aggregated rasters are not "
                                "verified)\n"),
}


def _nothing_written(tmp_path):
    return not (tmp_path / "logs").exists() and not [f for f in os.listdir(tmp_path) if f.startswith("cn_rasters")]


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refused_before_any_gpu(tmp_path, zones, case):
    keys, args, env, stderr = REFUSALS[case]
    fill = dict(zones=zones, tmp=str(tmp_path))
    args = [a.format(**fill) for a in args]
    if keys is not None:
        args = ["-c", _config(tmp_path, **keys)] + args
    p = _gcn10(args, tmp_path, env)
    assert p.returncode == 1, p.stdout + p.stderr
    assert p.stderr == stderr.format(**fill)
    assert p.stdout == ""
    assert _nothing_written(tmp_path)


# ---- a GPU library without an optional entry point: the stub has none of them ----------------------------------

@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("stub") / "libstub_gpu.so")
    subprocess.run(["gcc", "-std=c11", "-O1", "-fPIC", "-shared", "-pthread", "-I" + os.path.join(ROOT, "include"),
                    "-o", so, os.path.join(ROOT, "tests", "stub_gpu", "stub_gpu.c"), "-lz"], check=True)
    return so


LACKS = {
    "cog": (["--cog"], "gcn10_gpu_overview_* (needed by cog=1)"),
    "stats": (["--stats"], "gcn10_gpu_pair_histogram (needed by stats=1)"),
    "zonal": (["--zones", "{zones}"], "gcn10_gpu_zonal_pair_histogram (needed by zonal=1)"),
    "aggregate": (["--aggregate", "25"], "gcn10_gpu_aggregate (needed by aggregate=25)"),
    "verify": (["--verify"], "gcn10_gpu_verify_strip (needed by verify=1)"),
    "lzw": (["--compress", "lzw"], "gcn10_gpu_lzw_strip (needed by compress=lzw)"),
    # the first mode in the order cog, stats, zonal, aggregate, verify, lzw speaks
    "cog and stats and lzw": (["--compress", "lzw", "--stats", "--cog"], "gcn10_gpu_overview_* (needed by cog=1)"),
    "stats and verify": (["--verify", "--stats"], "gcn10_gpu_pair_histogram (needed by stats=1)"),
    # an aggregate run carries neither overviews nor statistics: neither is asked of the library
    "aggregate with cog and stats": (["--aggregate", "2", "--cog", "--stats"],
                                     "gcn10_gpu_aggregate (needed by aggregate=2)"),
}


@pytest.mark.parametrize("case", sorted(LACKS))
def test_a_gpu_library_without_the_entry_point_fails_at_start(tmp_path, zones, stub, case):
    args, what = LACKS[case]
    args = [a.format(zones=zones) for a in args]
    p = _gcn10(["-c", _config(tmp_path)] + args, tmp_path, {"GCN10_GPU_LIB": stub})
    assert p.returncode == 1, p.stdout + p.stderr
    assert p.stderr == "[rank 0] %s lacks %s\n" % (stub, what)
    assert p.stdout == ""
    assert _nothing_written(tmp_path)
