"""The compress option of the gcn10 program (config key "compress", --compress): values are checked at
config load, before anything needs a GPU, and LZW has no host encoder to fall back on."""
import os
import subprocess

import pytest

from gcn10_amd import host
from tests.conftest import LOOKUPS, ROOT

GCN10 = os.path.join(ROOT, "bin", "gcn10")
BASE = "hysogs_data_path=a\nesa_data_path=b\nblocks_shp_path=c\nlookup_table_path=%s\nlog_dir=%s\n"


def _cfg(tmp_path, extra):
    (tmp_path / "config.txt").write_text(BASE % (LOOKUPS, tmp_path / "logs") + extra)
    return str(tmp_path / "config.txt")


def _run(tmp_path, *args):
    return subprocess.run([GCN10, *args], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)


def test_help_lists_compress():
    out = subprocess.run([GCN10, "-h"], capture_output=True, text=True)
    assert out.returncode == 0 and "--compress <c>" in out.stdout and "deflate or lzw" in out.stdout


def test_unknown_compress_value_in_config_exits_1(tmp_path):
    _cfg(tmp_path, "compress=zstd\n")
    out = _run(tmp_path, "-c", "config.txt")
    assert out.returncode == 1
    assert "bad value for compress: 'zstd' (deflate or lzw)" in out.stderr


def test_unknown_compress_value_on_the_command_line_exits_1(tmp_path):
    _cfg(tmp_path, "")
    out = _run(tmp_path, "-c", "config.txt", "--compress", "bogus")
    assert out.returncode == 1
    assert "bad value for compress: 'bogus' (deflate or lzw)" in out.stderr


@pytest.mark.parametrize("where", ["config", "cli"])
def test_lzw_without_gpu_encoding_is_refused(tmp_path, where):
    _cfg(tmp_path, "gpu_deflate=0\n" + ("compress=lzw\n" if where == "config" else ""))
    out = _run(tmp_path, "-c", "config.txt", *(["--compress", "lzw"] if where == "cli" else []))
    assert out.returncode == 1
    assert "bad value for compress: 'lzw'" in out.stderr and "gpu_deflate=0" in out.stderr
    assert "no CPU fallback" not in out.stderr          # refused at config load, not when the GPU is sought


def test_config_values_are_case_insensitive(tmp_path):
    p = _cfg(tmp_path, "")
    assert host.parse_config(p)["compress"] == 0                     # absent = deflate
    for val, want in (("deflate", 0), ("DEFLATE", 0), ("lzw", 1), ("LZW", 1), ("Lzw", 1)):
        p = _cfg(tmp_path, "compress=%s\n" % val)
        assert host.parse_config(p)["compress"] == want, val
    p = _cfg(tmp_path, "compress=packbits\n")
    with pytest.raises(host.HostError, match=r"bad value for compress: 'packbits' \(deflate or lzw\)"):
        host.parse_config(p)
