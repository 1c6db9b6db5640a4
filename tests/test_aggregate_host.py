"""CPU: the host side of the aggregate run mode (config key aggregate, --aggregate): the geometry of a block's grid
of cells (gcn10_aggregate_geometry), config parsing, the combinations refused before any GPU is touched, and the
start-up failure with a GPU library that lacks gcn10_gpu_aggregate (the stub of tests/stub_gpu)."""
import math
import os
import subprocess

import numpy as np
import pytest

from gcn10_amd import host
from oracle import cn_oracle_c as oc
from tests import zoneutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PX = 8.3333333333330430e-05         # the landcover's pixel size


def _config(tmp_path, **extra):
    p = tmp_path / "cfg.txt"
    keys = dict(hysogs_data_path="h", esa_data_path="e", blocks_shp_path="b", lookup_table_path="l",
                log_dir=str(tmp_path / "logs"))
    keys.update({k: str(v) for k, v in extra.items()})
    p.write_text("".join("%s=%s\n" % kv for kv in keys.items()))
    return str(p)


def _gcn10(args, cwd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([os.path.join(ROOT, "bin", "gcn10")] + args, cwd=str(cwd), capture_output=True, text=True,
                          timeout=120, env=e)


# ---- geometry -----------------------------------------------------------------------------------------------------

def _model(W, H, gt, own, f):
    """The definition in numpy: the owned rectangle from the ownership mask of tests/zoneutil.py."""
    m = zoneutil.own_mask(gt, W, H, own) if own is not None else np.ones((H, W), bool)
    xs, ys = np.flatnonzero(m.any(axis=0)), np.flatnonzero(m.any(axis=1))
    x0, x1, y0, y1 = int(xs[0]), int(xs[-1]) + 1, int(ys[0]), int(ys[-1]) + 1
    assert m[y0:y1, x0:x1].all() and m.sum() == (x1 - x0) * (y1 - y0)
    return dict(x0=x0, x1=x1, y0=y0, y1=y1, Wa=-(-(x1 - x0) // f), Ha=-(-(y1 - y0) // f),
                gt=[gt[0] + x0 * gt[1], f * gt[1], 0.0, gt[3] + y0 * gt[5], 0.0, f * gt[5]])


def _same(got, want):
    assert {k: got[k] for k in ("x0", "x1", "y0", "y1", "Wa", "Ha")} == {k: want[k] for k in want if k != "gt"}
    assert got["gt"].tolist() == want["gt"]         # the six doubles, exactly


VRT_GT = [-180.0, PX, 0.0, 84.0, 0.0, -PX]         # the landcover mosaic's geotransform, 4320000 x 1728000 px


def test_a_real_block_gives_1440_cells_a_side_at_25():
    """A 3 degree block of the real mosaic: its window is 36001 px a side (the pixel size is a little under 1 / 12000
    degree) and shares a pixel row and column with its neighbours; the block owns 36000 x 36000 of it."""
    own = [-111.0, 36.0, -108.0, 39.0]
    _xo, _yo, W, H, gt = oc.window(VRT_GT, 4320000, 1728000, own)
    assert (W, H) == (36001, 36001)
    px = gt[0] + (np.arange(W) + 0.5) * gt[1]
    py = gt[3] + (np.arange(H) + 0.5) * gt[5]
    x = np.flatnonzero((px >= own[0]) & (px < own[2]))
    y = np.flatnonzero((py > own[1]) & (py <= own[3]))
    g = host.aggregate_geometry(W, H, gt, own, 25)
    assert (g["x0"], g["x1"], g["y0"], g["y1"]) == (x[0], x[-1] + 1, y[0], y[-1] + 1)
    assert g["x1"] - g["x0"] == 36000 and g["y1"] - g["y0"] == 36000
    assert (g["Wa"], g["Ha"]) == (1440, 1440)
    assert g["gt"].tolist() == [gt[0] + g["x0"] * PX, 25 * PX, 0.0, gt[3] + g["y0"] * -PX, 0.0, 25 * -PX]
    g100 = host.aggregate_geometry(W, H, gt, own, 100)
    assert (g100["Wa"], g100["Ha"]) == (360, 360) and g100["gt"][1] == 100 * PX
    # the neighbour to the east begins where this block ends: no cell is shared, none is left out
    east = [-108.0, 36.0, -105.0, 39.0]
    xo2, _yo2, W2, H2, gt2 = oc.window(VRT_GT, 4320000, 1728000, east)
    g2 = host.aggregate_geometry(W2, H2, gt2, east, 25)
    assert _xo + g["x1"] == xo2 + g2["x0"]


@pytest.mark.parametrize("f", [2, 7, 25, 256])
def test_blocks_with_and_without_overlap(f):
    gt = [10.0, PX, 0.0, 50.0, 0.0, -PX]
    W, H = 337, 481
    # no box, a box that is the window, and boxes that cut a pixel column / row off either side
    _same(host.aggregate_geometry(W, H, gt, None, f), _model(W, H, gt, None, f))
    whole = [gt[0], gt[3] + H * gt[5], gt[0] + W * gt[1], gt[3]]
    _same(host.aggregate_geometry(W, H, gt, whole, f), _model(W, H, gt, whole, f))
    assert host.aggregate_geometry(W, H, gt, whole, f)["Wa"] == math.ceil(W / f)
    for own in ([10.0 + 0.6 * PX, 50.0 - 479.4 * PX, 10.0 + 336.2 * PX, 50.0 - 1.3 * PX],
                [10.0 + 0.5 * PX, 50.0 - 480.5 * PX, 10.0 + 336.5 * PX, 50.0 - 0.5 * PX],     # edges ON pixel centres
                [9.0, 49.0, 10.0 + 100 * PX, 50.0 - 7 * PX]):
        _same(host.aggregate_geometry(W, H, gt, own, f), _model(W, H, gt, own, f))


def test_a_block_narrower_than_a_cell_is_one_column_of_cells():
    gt = [10.0, PX, 0.0, 50.0, 0.0, -PX]
    g = host.aggregate_geometry(17, 60, gt, None, 25)
    assert (g["Wa"], g["Ha"]) == (1, 3) and g["gt"][1] == 25 * PX
    g = host.aggregate_geometry(3, 2, gt, None, 256)
    assert (g["Wa"], g["Ha"], g["x0"], g["x1"], g["y0"], g["y1"]) == (1, 1, 0, 3, 0, 2)


@pytest.mark.parametrize("args", [dict(f=1), dict(f=257), dict(f=0), dict(gt=[10.0, PX, 0.0, 50.0, 0.0, PX]),
                                  dict(gt=[10.0, PX, 1e-9, 50.0, 0.0, -PX]), dict(own=[20.0, 49.0, 21.0, 50.0]),
                                  dict(W=0)])
def test_geometry_refuses(args):
    kw = dict(W=100, H=100, gt=[10.0, PX, 0.0, 50.0, 0.0, -PX], own=None, f=25)
    kw.update(args)
    with pytest.raises(host.HostError):
        host.aggregate_geometry(kw["W"], kw["H"], kw["gt"], kw["own"], kw["f"])


# ---- config and command line --------------------------------------------------------------------------------------

def test_the_key_parses_and_the_default_is_off(tmp_path):
    assert host.parse_config(_config(tmp_path))["aggregate"] == 0
    for v in (0, 2, 25, 100, 256):
        assert host.parse_config(_config(tmp_path, aggregate=v))["aggregate"] == v
    # appended behind every field the struct had before
    assert [n for n, _t in host.ConfigFull._fields_][-1] == "aggregate"


@pytest.mark.parametrize("value", ["1", "257", "-2", "25.0", "x", "", "2 5", "1000"])
def test_config_refuses_bad_values(tmp_path, value):
    with pytest.raises(host.HostError, match=r"bad value for aggregate: '%s' \(0 or an integer 2\.\.256\)" % value):
        host.parse_config(_config(tmp_path, aggregate=value))


def test_cli_help_lists_the_flag():
    p = _gcn10(["-h"], ROOT)
    assert p.returncode == 0 and "--aggregate <f>" in p.stdout and "cn_rasters_<cond>_x<f>" in p.stdout


@pytest.mark.parametrize("case,msg", [
    ("bad flag", "bad value for aggregate: '1' (0 or an integer 2..256)"),
    ("bad key", "bad value for aggregate: '300'"),
    ("verify flag", "aggregate cannot be combined with --verify"),
    ("verify key", "aggregate cannot be combined with --verify"),
    ("zonal", "aggregate cannot be combined with --zonal"),
])
def test_cli_refuses_before_any_gpu(tmp_path, case, msg):
    extra, args = {}, []
    if case == "bad flag":
        args = ["--aggregate", "1"]
    elif case == "bad key":
        extra = dict(aggregate=300)
    elif case == "verify flag":
        args = ["--aggregate", "25", "--verify"]
    elif case == "verify key":
        extra = dict(aggregate=25, verify=1)
    elif case == "zonal":
        zoneutil.write_zone_shapefile(str(tmp_path / "zones"), [(1, [[(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]])])
        extra, args = dict(aggregate=7), ["--zones", str(tmp_path / "zones.shp")]
    p = _gcn10(["-c", _config(tmp_path, **extra)] + args, tmp_path)
    assert p.returncode == 1, p.stdout + p.stderr
    assert msg in p.stderr
    assert "no CPU fallback" not in p.stderr        # refused at start, not when the GPU is sought
    assert not (tmp_path / "logs").exists() and not [f for f in os.listdir(tmp_path) if f.startswith("cn_rasters")]


def test_a_gpu_library_without_the_symbol_fails_at_start(tmp_path):
    stub = str(tmp_path / "libstub_gpu.so")
    subprocess.run(["gcc", "-std=c11", "-O1", "-fPIC", "-shared", "-pthread", "-I" + os.path.join(ROOT, "include"),
                    "-o", stub, os.path.join(ROOT, "tests", "stub_gpu", "stub_gpu.c"), "-lz"], check=True)
    p = _gcn10(["-c", _config(tmp_path), "--aggregate", "25"], tmp_path, {"GCN10_GPU_LIB": stub})
    assert p.returncode == 1, p.stdout + p.stderr
    assert "lacks gcn10_gpu_aggregate (needed by aggregate=25)" in p.stderr and stub in p.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("cn_rasters")]
    # the same library serves a run that does not aggregate as far as it ever did: no such complaint
    q = _gcn10(["-c", _config(tmp_path)], tmp_path, {"GCN10_GPU_LIB": stub})
    assert "gcn10_gpu_aggregate" not in q.stderr
