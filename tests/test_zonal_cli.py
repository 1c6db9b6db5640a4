"""CPU: the config keys and command-line flags of the zonal run mode (zonal, zones_shp_path, zones_id_field,
zonal_output; --zonal, --zones): parsing, the help text, and the combinations refused before any GPU is touched."""
import os
import subprocess

import pytest

from gcn10_amd import host
from tests import zoneutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQUARE = [[(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]]


def _config(tmp_path, **extra):
    p = tmp_path / "cfg.txt"
    keys = dict(hysogs_data_path="h", esa_data_path="e", blocks_shp_path="b", lookup_table_path="l",
                log_dir=str(tmp_path / "logs"))
    keys.update({k: str(v) for k, v in extra.items()})
    p.write_text("".join("%s=%s\n" % kv for kv in keys.items()))
    return str(p)


def _gcn10(args, cwd, env=None):
    exe = os.path.join(ROOT, "bin", "gcn10")
    e = dict(os.environ)
    for k in ("OMPI_COMM_WORLD_RANK", "OMPI_COMM_WORLD_SIZE", "PMI_RANK", "PMI_SIZE", "PMIX_RANK", "PMIX_SIZE",
              "SLURM_PROCID", "SLURM_NTASKS"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([exe] + args, cwd=str(cwd), capture_output=True, text=True, timeout=120, env=e)


@pytest.fixture()
def zones(tmp_path):
    zoneutil.write_zone_shapefile(str(tmp_path / "zones"), [(1, SQUARE)])
    return str(tmp_path / "zones.shp")


def test_defaults_leave_the_mode_off(tmp_path):
    cfg = host.parse_config(_config(tmp_path))
    assert cfg["zonal"] == 0 and cfg["zones_shp_path"] is None and cfg["zones_id_field"] is None
    assert cfg["zonal_output"] is None
    # the new fields come after every field the struct had before
    assert [n for n, _t in host.ConfigFull._fields_][:2] == ["verify", "zonal"]


def test_the_keys_parse(tmp_path):
    cfg = host.parse_config(_config(tmp_path, zonal=1, zones_shp_path="/data/basins.shp", zones_id_field="HYBAS_ID",
                                    zonal_output="out/table.csv", lookups="g_ii", conditions="drained"))
    assert cfg["zonal"] == 1 and cfg["zones_shp_path"] == "/data/basins.shp"
    assert cfg["zones_id_field"] == "HYBAS_ID" and cfg["zonal_output"] == "out/table.csv"
    assert cfg["table_mask"] == 1 << 7 and cfg["cond_mask"] == 1
    assert host.parse_config(_config(tmp_path, zonal=0))["zonal"] == 0


@pytest.mark.parametrize("extra,msg", [(dict(zonal="2"), "bad value for zonal: '2' (0 or 1)"),
                                       (dict(zonal="yes"), "bad value for zonal"),
                                       (dict(zonal=""), "bad value for zonal"),
                                       (dict(zones_id_field=""), "bad value for zones_id_field"),
                                       (dict(zones_id_field="ELEVEN_CHARS"), "bad value for zones_id_field: 'ELEVEN_CHARS'")])
def test_config_refuses(tmp_path, extra, msg):
    with pytest.raises(host.HostError, match=msg.replace("(", r"\(").replace(")", r"\)")):
        host.parse_config(_config(tmp_path, **extra))


def test_cli_help_lists_the_flags():
    p = _gcn10(["-h"], ROOT)
    assert p.returncode == 0
    assert "--zonal" in p.stdout and "--zones <file.shp>" in p.stdout and "zonal_cn.csv" in p.stdout


@pytest.mark.parametrize("case,msg", [
    ("no zones", "zonal=1 needs the zone polygons"),
    ("no zones, key", "zonal=1 needs the zone polygons"),
    ("overwrite", "cannot be combined with --overwrite"),
    ("verify flag", "cannot be combined with --verify"),
    ("verify key", "cannot be combined with --verify"),
    ("ompi", "merging tables across launcher ranks is not supported"),
    ("pmi", "merging tables across launcher ranks is not supported"),
    ("slurm", "merging tables across launcher ranks is not supported"),
    ("bad key", "bad value for zonal"),
    ("missing file", "not a shapefile"),
    ("missing field", 'no "BASIN" field'),
])
def test_cli_refuses_before_any_gpu(tmp_path, zones, case, msg):
    extra, args, env = {}, [], {}
    if case == "no zones":
        args = ["--zonal"]
    elif case == "no zones, key":
        extra = dict(zonal=1)
    elif case == "overwrite":
        args = ["--zones", zones, "--overwrite"]
    elif case == "verify flag":
        args = ["--zones", zones, "--verify"]
    elif case == "verify key":
        extra = dict(zonal=1, zones_shp_path=zones, verify=1)
    elif case == "ompi":
        args, env = ["--zones", zones], {"OMPI_COMM_WORLD_RANK": "1", "OMPI_COMM_WORLD_SIZE": "2"}
    elif case == "pmi":
        args, env = ["--zones", zones], {"PMI_RANK": "0", "PMI_SIZE": "4"}
    elif case == "slurm":
        extra, env = dict(zonal=1, zones_shp_path=zones), {"SLURM_PROCID": "0", "SLURM_NTASKS": "2"}
    elif case == "bad key":
        extra = dict(zonal="3", zones_shp_path=zones)
    elif case == "missing file":
        args = ["--zones", str(tmp_path / "nothing.shp")]
    elif case == "missing field":
        extra, args = dict(zones_id_field="BASIN"), ["--zones", zones]
    p = _gcn10(["-c", _config(tmp_path, **extra)] + args, tmp_path, env)
    assert p.returncode == 1, p.stdout + p.stderr
    assert msg in p.stderr
    assert "no CPU fallback" not in p.stderr        # refused at start, not when the GPU is sought
    assert not (tmp_path / "zonal_cn.csv").exists() and not (tmp_path / "logs").exists()


def test_a_launcher_of_one_rank_is_no_refusal(tmp_path, zones):
    """size 1 is a plain run: it gets as far as looking for the GPU (or further where there is one)."""
    p = _gcn10(["-c", _config(tmp_path), "--zones", zones], tmp_path, {"SLURM_PROCID": "0", "SLURM_NTASKS": "1"})
    assert "launcher ranks" not in p.stderr and "needs the zone polygons" not in p.stderr
