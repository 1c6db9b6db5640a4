"""CPU: the config keys and command-line flags of the band statistics (stats, nodata): parsing, refusals at config
load, and the help text."""
import os
import subprocess

import pytest

from gcn10_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _config(tmp_path, **extra):
    p = tmp_path / "cfg.txt"
    keys = dict(hysogs_data_path="h", esa_data_path="e", blocks_shp_path="b", lookup_table_path="l", log_dir="d")
    keys.update({k: str(v) for k, v in extra.items()})
    p.write_text("".join("%s=%s\n" % kv for kv in keys.items()))
    return str(p)


def _gcn10(args, cwd):
    exe = os.path.join(ROOT, "bin", "gcn10")
    return subprocess.run([exe] + args, cwd=cwd, capture_output=True, text=True, timeout=120)


def test_defaults_leave_both_off(tmp_path):
    cfg = host.parse_config(_config(tmp_path))
    assert cfg["stats"] == 0 and cfg["nodata"] == -1
    # the new fields come after every field the struct had before
    names = [n for n, _t in host.Config._fields_]
    assert names[-3:] == ["overview_resampling", "stats", "nodata"]


@pytest.mark.parametrize("stats,nodata,want", [("1", "255", (1, 255)), ("0", "0", (0, 0)), ("1", "none", (1, -1)),
                                               ("0", "NONE", (0, -1)), ("1", "007", (1, 7)), ("1", "100", (1, 100))])
def test_config_accepts(tmp_path, stats, nodata, want):
    cfg = host.parse_config(_config(tmp_path, stats=stats, nodata=nodata))
    assert (cfg["stats"], cfg["nodata"]) == want


@pytest.mark.parametrize("extra,msg", [(dict(stats="2"), "bad value for stats: '2' (0 or 1)"),
                                       (dict(stats="yes"), "bad value for stats"),
                                       (dict(stats=""), "bad value for stats"),
                                       (dict(nodata="256"), "bad value for nodata: '256'"),
                                       (dict(nodata="-1"), "bad value for nodata"),
                                       (dict(nodata="12a"), "bad value for nodata"),
                                       (dict(nodata="0255"), "bad value for nodata"),
                                       (dict(nodata=""), "bad value for nodata"),
                                       (dict(nodata="nan"), "bad value for nodata")])
def test_config_refuses(tmp_path, extra, msg):
    with pytest.raises(host.HostError, match=msg.replace("(", r"\(").replace(")", r"\)")):
        host.parse_config(_config(tmp_path, **extra))


def test_cli_help_lists_the_flags():
    p = _gcn10(["-h"], ROOT)
    assert p.returncode == 0
    assert "--stats" in p.stdout and "--nodata" in p.stdout


@pytest.mark.parametrize("cfg_extra,args,msg", [
    (dict(stats="3"), [], "bad value for stats"),
    (dict(nodata="300"), [], "bad value for nodata"),
    ({}, ["--nodata", "x"], "bad value for nodata: 'x'"),
    ({}, ["--stats", "--nodata", "-5"], "bad value for nodata"),
    (dict(nodata="255"), ["--nodata", "256"], "bad value for nodata"),
])
def test_cli_refuses_before_any_gpu(tmp_path, cfg_extra, args, msg):
    cfg = _config(tmp_path, log_dir=str(tmp_path / "logs"), **cfg_extra)
    p = _gcn10(["-c", cfg] + args, str(tmp_path))
    assert p.returncode == 1, p.stdout + p.stderr
    assert msg in p.stderr
    assert "no CPU fallback" not in p.stderr        # refused at config load, not when the GPU is sought
