"""The host side of the verification mode without a GPU: the option (--verify, config key verify), what is refused
before a GPU is sought, and the structure checks a verify run makes on an output raster before any pixel work
(gcn10_verify_structure), one malformed file per finding.  The files come from tests/tiffutil.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

from gcn10_amd import host
from tests import tiffutil
from tests.conftest import LOOKUPS, ROOT

GCN10 = os.path.join(ROOT, "bin", "gcn10")
BASE = "hysogs_data_path=a\nesa_data_path=b\nblocks_shp_path=c\nlookup_table_path=%s\nlog_dir=%s\n"
GT = [10.25, 0.001, 0.0, 49.5, 0.0, -0.001]


def _cfg(tmp_path, extra):
    (tmp_path / "config.txt").write_text(BASE % (LOOKUPS, tmp_path / "logs") + extra)
    return str(tmp_path / "config.txt")


def _run(tmp_path, *args):
    return subprocess.run([GCN10, *args], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)


def patch_ifd(path, ifd_index, tag, value):
    """Overwrites the inline value of a SHORT or LONG entry with count 1 in directory `ifd_index` of a classic
    little-endian TIFF."""
    with open(path, "r+b") as f:
        data = f.read()
        assert data[:4] == b"II*\0"
        pos = struct.unpack_from("<I", data, 4)[0]
        for _ in range(ifd_index):
            n = struct.unpack_from("<H", data, pos)[0]
            pos = struct.unpack_from("<I", data, pos + 2 + 12 * n)[0]
            assert pos, "no such directory"
        n = struct.unpack_from("<H", data, pos)[0]
        for i in range(n):
            e = pos + 2 + 12 * i
            t, typ, count = struct.unpack_from("<HHI", data, e)
            if t == tag:
                assert count == 1 and typ in (3, 4)
                f.seek(e + 8)
                f.write(struct.pack("<H" if typ == 3 else "<I", value))
                return
    raise AssertionError("tag %d not found" % tag)


def img(h=300, w=520, seed=1):
    return np.random.default_rng(seed).integers(0, 101, size=(h, w), dtype=np.uint8)


# ---- the option ------------------------------------------------------------------------------------------------

def test_help_lists_verify():
    out = subprocess.run([GCN10, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--verify" in out.stdout and "verify_failed_blocks.txt" in out.stdout


def test_config_key_verify(tmp_path):
    assert host.parse_config(_cfg(tmp_path, ""))["verify"] == 0
    assert host.parse_config(_cfg(tmp_path, "verify=1\n"))["verify"] == 1
    assert host.parse_config(_cfg(tmp_path, "verify=0\n"))["verify"] == 0
    for bad in ("2", "yes", "-1", ""):
        with pytest.raises(host.HostError, match=r"bad value for verify: '%s' \(0 or 1\)" % bad):
            host.parse_config(_cfg(tmp_path, "verify=%s\n" % bad))


def test_bad_verify_value_exits_1(tmp_path):
    _cfg(tmp_path, "verify=2\n")
    out = _run(tmp_path, "-c", "config.txt")
    assert out.returncode == 1
    assert "bad value for verify: '2' (0 or 1)" in out.stderr


@pytest.mark.parametrize("where", ["cli", "config"])
def test_verify_with_overwrite_is_refused_before_a_gpu_is_sought(tmp_path, where):
    _cfg(tmp_path, "verify=1\n" if where == "config" else "")
    out = _run(tmp_path, "-c", "config.txt", "--overwrite", *(["--verify"] if where == "cli" else []))
    assert out.returncode == 1
    assert "--verify writes nothing and cannot be combined with --overwrite" in out.stderr
    assert "no CPU fallback" not in out.stderr and "cannot load" not in out.stderr
    assert not (tmp_path / "logs").exists()


# ---- the structure of one file -----------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", [dict(compression=8, tile=(256, 256)), dict(compression=5, rows_per_strip=37, predictor=2),
                                    dict(compression=1), dict(compression=8, tile=(512, 512), bigtiff=True)])
def test_good_files_have_no_finding(tmp_path, layout):
    p = str(tmp_path / "a.tif")
    tiffutil.write_tiff(p, img(), gt=GT, **layout)
    r = host.verify_structure(p, 520, 300, GT)
    assert (r["finding"], r["code"], r["n_levels"]) == ("ok", 0, 0), r


def test_missing_file(tmp_path):
    r = host.verify_structure(str(tmp_path / "none.tif"), 520, 300, GT)
    assert r["finding"] == "missing" and r["code"] == 1


def test_not_a_tiff(tmp_path):
    p = tmp_path / "a.tif"
    p.write_bytes(b"GIF89a" + bytes(200))
    assert host.verify_structure(str(p), 520, 300, GT)["finding"] == "not a TIFF"
    p.write_bytes(b"")
    assert host.verify_structure(str(p), 520, 300, GT)["finding"] == "not a TIFF"
    # a TIFF cut inside its directory
    tiffutil.write_tiff(str(p), img(), gt=GT, compression=8, tile=(256, 256))
    data = p.read_bytes()
    p.write_bytes(data[:struct.unpack_from("<I", data, 4)[0] + 20])
    assert host.verify_structure(str(p), 520, 300, GT)["finding"] == "not a TIFF"


def test_not_one_band_of_byte(tmp_path):
    p = str(tmp_path / "a.tif")
    tiffutil.write_tiff(p, img(), gt=GT, compression=1)
    patch_ifd(p, 0, 258, 16)                    # BitsPerSample
    r = host.verify_structure(p, 520, 300, GT)
    assert r["finding"] == "not 1 band Byte" and "16 bits" in r["reason"], r
    tiffutil.write_tiff(p, np.repeat(img(), 3, axis=1), gt=GT, compression=1)
    patch_ifd(p, 0, 256, 520)
    patch_ifd(p, 0, 277, 3)                     # SamplesPerPixel: the same bytes as three bands
    r = host.verify_structure(p, 520, 300, GT)
    assert r["finding"] == "not 1 band Byte" and "3 samples" in r["reason"], r


def test_wrong_size(tmp_path):
    p = str(tmp_path / "a.tif")
    tiffutil.write_tiff(p, img()[:, :-1], gt=GT, compression=8, tile=(256, 256))
    r = host.verify_structure(p, 520, 300, GT)
    assert r["finding"] == "size" and "519x300" in r["reason"] and "520x300" in r["reason"], r
    assert host.verify_structure(p, 519, 300, GT)["finding"] == "ok"
    assert host.verify_structure(p, 519, 301, GT)["finding"] == "size"


@pytest.mark.parametrize("i,delta", [(0, 0.001), (3, -0.001), (1, 1e-12), (5, 1e-12), (0, 2e-15)])
def test_shifted_geotransform(tmp_path, i, delta):
    p = str(tmp_path / "a.tif")
    gt = list(GT)
    gt[i] += delta
    assert gt[i] != GT[i]
    tiffutil.write_tiff(p, img(), gt=gt, compression=8, tile=(256, 256))
    r = host.verify_structure(p, 520, 300, GT)
    assert r["finding"] == "geotransform", r
    assert host.verify_structure(p, 520, 300, gt)["finding"] == "ok"


def test_chunk_beyond_the_end_of_the_file(tmp_path):
    # directories in front of the data, as in the program's COGs: cutting the file leaves them whole
    p = tmp_path / "a.tif"
    tiffutil.write_cog(str(p), img(600, 700), gt=GT, tile=(256, 256), overviews=0)
    assert host.verify_structure(str(p), 700, 600, GT)["finding"] == "ok"
    data = p.read_bytes()
    p.write_bytes(data[:len(data) * 2 // 3])
    r = host.verify_structure(str(p), 700, 600, GT)
    assert r["finding"] == "chunk" and "beyond the end of the file" in r["reason"], r


def test_chunk_without_bytes(tmp_path):
    p = str(tmp_path / "a.tif")
    tiffutil.write_tiff(p, img(100, 120), gt=GT, compression=8)            # one strip: its count is an inline value
    assert host.verify_structure(p, 120, 100, GT)["finding"] == "ok"
    patch_ifd(p, 0, 279, 0)
    r = host.verify_structure(p, 120, 100, GT)
    assert r["finding"] == "chunk" and "no bytes" in r["reason"], r


def test_overview_directories(tmp_path):
    p = str(tmp_path / "a.tif")
    tiffutil.write_cog(p, img(601, 701), gt=GT, tile=(256, 256), overviews=2)     # 351 x 301, 176 x 151
    r = host.verify_structure(p, 701, 601, GT)
    assert (r["finding"], r["n_levels"]) == ("ok", 2), r
    patch_ifd(p, 2, 256, 175)
    r = host.verify_structure(p, 701, 601, GT)
    assert r["finding"] == "overview size" and "overview 2" in r["reason"] and "176x151" in r["reason"], r
