"""CPU: the COG writer (gcn10_tiff_create_cog and the level views of the put calls), the level-count rule, and the
config / command-line rules of cog and overview_resampling."""
import math
import os
import subprocess
import zlib

import numpy as np
import pytest
from PIL import Image

from gcn10_amd import host
from tests import cogcheck
from tests.tiffutil import lzw_encode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GT = [10.0, 0.001, 0.0, 50.0, 0.0, -0.001]


def level_image(W, H, k, seed):
    w, h = math.ceil(W / 2 ** k), math.ceil(H / 2 ** k)
    rng = np.random.default_rng(seed * 31 + k)
    img = ((np.arange(w)[None, :] // 7 + np.arange(h)[:, None] // 5 + k * 13) % 97).astype(np.uint8)
    img[rng.random((h, w)) < 0.05] = 255
    return img


def tile_of(img, tx, ty):
    t = np.zeros((256, 256), np.uint8)
    part = img[ty * 256:(ty + 1) * 256, tx * 256:(tx + 1) * 256]
    t[:part.shape[0], :part.shape[1]] = part
    return t.tobytes()


def write_cog(path, W, H, compression, direct, seed=0, extents=True):
    L = host.cog_levels(W, H)
    enc = (lambda b: zlib.compress(b, 6)) if compression == 8 else lzw_encode
    wr = host.TiffWriter(path, W, H, GT, n_levels=L, compression=compression, direct=direct)
    imgs = {}
    try:
        for k in range(L, -1, -1):
            imgs[k] = img = level_image(W, H, k, seed)
            across, down = wr.tiles(k)
            assert (across, down) == (math.ceil(img.shape[1] / 256), math.ceil(img.shape[0] / 256))
            for ty in range(down):
                row = [(tx, ty, enc(tile_of(img, tx, ty))) for tx in range(across)]
                if extents and ty % 2 == 0:     # extents and single puts by turns, with or without O_DIRECT
                    assert wr.put_extent(row, level=k) == 0
                else:
                    for tx, _ty, d in row:
                        assert wr.put_tile(tx, ty, d, level=k) == 0
        wr.finish()
    except BaseException:
        wr.abort()
        raise
    return L, imgs


def pil_levels(path):
    out = []
    with Image.open(path) as im:
        k = 0
        while True:
            try:
                im.seek(k)
            except EOFError:
                break
            out.append(np.array(im))
            k += 1
    return out


ROUND_TRIPS = [(W, H, c, d) for W, H in [(1, 1), (256, 256), (257, 3), (513, 700)] for c in (8, 5)
               for d in (False, True)] + [(36001, 300, 8, False), (36001, 300, 5, True)]


@pytest.mark.parametrize("W,H,compression,direct", ROUND_TRIPS)
def test_cog_round_trip(tmp_path, W, H, compression, direct):
    path = str(tmp_path / "cog.tif")
    L, imgs = write_cog(path, W, H, compression, direct, seed=W + H)
    assert not os.path.exists(path + ".part")
    ifds = cogcheck.check_cog(path, n_levels=L, compression=compression)
    # every level decodes back to its input through PIL (libtiff)
    levels = pil_levels(path)
    assert len(levels) == L + 1
    for k in range(L + 1):
        np.testing.assert_array_equal(levels[k], imgs[k], err_msg="level %d" % k)
    # the host reader takes the full-resolution IFD
    with host.Raster(path) as r:
        np.testing.assert_array_equal(r.read(0, 0, W, H), imgs[0])
    # the main IFD is the plain writer's tag set, geo tags included
    assert {33550, 33922, 34735} <= set(ifds[0][2])


def test_plain_writer_unchanged_by_cog_views(tmp_path):
    """A plain file has no ghost area, its IFD after the data, and takes puts in any order."""
    path = str(tmp_path / "plain.tif")
    img = level_image(600, 300, 0, 1)
    wr = host.TiffWriter(path, 600, 300, GT)
    assert wr.n_levels == 0
    for ty in reversed(range(2)):
        for tx in reversed(range(3)):
            assert wr.put_tile(tx, ty, zlib.compress(tile_of(img, tx, ty))) == 0
    wr.finish()
    data = open(path, "rb").read()
    assert b"GDAL_STRUCTURAL_METADATA_SIZE" not in data[:200]
    with host.Raster(path) as r:
        np.testing.assert_array_equal(r.read(0, 0, 600, 300), img)


def test_out_of_order_puts_are_refused(tmp_path):
    W, H = 700, 513                         # levels: 350x257 (2x2 tiles), 175x129 (1 tile)
    path = str(tmp_path / "cog.tif")
    wr = host.TiffWriter(path, W, H, GT, n_levels=host.cog_levels(W, H))
    assert wr.n_levels == 2
    z = {k: level_image(W, H, k, 3) for k in range(3)}
    t = lambda k, tx, ty: zlib.compress(tile_of(z[k], tx, ty))
    try:
        assert wr.put_tile(0, 0, t(1, 0, 0), level=1) == 0      # level 2 may not come after level 1 ...
        assert wr.put_tile(0, 0, t(2, 0, 0), level=2) == -1
        assert wr.put_tile(1, 0, t(1, 1, 0), level=1) == 0
        assert wr.put_tile(0, 0, t(1, 0, 0), level=1) == -1     # ... nor a tile before the last one of its level
        assert wr.put_tile(1, 0, t(1, 1, 0), level=1) == -1     # ... nor the same one again
        # an extent whose streams are not in row-major order, or not at increasing positions
        assert wr.put_extent([(1, 1, t(1, 1, 1)), (0, 1, t(1, 0, 1))], level=1) == -1
        with pytest.raises(host.HostError):
            wr.tiles(3)
        # refusals leave the file usable; level 2 is then missing, so finish names it
        assert wr.put_extent([(0, 1, t(1, 0, 1)), (1, 1, t(1, 1, 1))], level=1) == 0
        for ty in range(3):
            for tx in range(3):
                assert wr.put_tile(tx, ty, t(0, tx, ty)) == 0
        assert wr.put_tile(0, 0, t(1, 0, 0), level=1) == -1     # back to a coarser level
    except BaseException:
        wr.abort()
        raise
    with pytest.raises(host.HostError, match="overview level 2"):
        wr.finish()
    assert not os.path.exists(path) and not os.path.exists(path + ".part")


def test_no_level_window_is_still_a_cog(tmp_path):
    path = str(tmp_path / "small.tif")
    L, imgs = write_cog(path, 200, 256, 8, False)
    assert L == 0
    ifds = cogcheck.check_cog(path, n_levels=0)
    assert len(ifds) == 1


@pytest.mark.parametrize("n,want", [(1, 0), (256, 0), (257, 1), (512, 1), (513, 2), (36000, 8), (36001, 8)])
def test_level_count_rule(n, want):
    assert host.cog_levels(n, n) == want
    assert host.cog_levels(n, 1) == want
    assert host.cog_levels(1, n) == want
    assert cogcheck.expected_levels(n, n) == want


def test_level_count_mixed_and_limits():
    assert host.cog_levels(65536, 10) == 8
    assert host.cog_levels(65537, 10) == 9
    assert host.cog_levels(0, 5) == -1


def _config(tmp_path, **extra):
    p = tmp_path / "cfg.txt"
    keys = dict(hysogs_data_path="h", esa_data_path="e", blocks_shp_path="b", lookup_table_path="l", log_dir="d")
    keys.update({k: str(v) for k, v in extra.items()})
    p.write_text("".join("%s=%s\n" % kv for kv in keys.items()))
    return str(p)


def test_config_defaults(tmp_path):
    cfg = host.parse_config(_config(tmp_path))
    assert cfg["cog"] == 0 and cfg["overview_resampling"] == 0


@pytest.mark.parametrize("cog,res,want", [("1", "nearest", (1, 0)), ("1", "AVERAGE", (1, 1)), ("0", "Average", (0, 1)),
                                          ("1", "Nearest", (1, 0))])
def test_config_accepts(tmp_path, cog, res, want):
    cfg = host.parse_config(_config(tmp_path, cog=cog, overview_resampling=res))
    assert (cfg["cog"], cfg["overview_resampling"]) == want


@pytest.mark.parametrize("extra,msg", [(dict(cog="2"), "bad value for cog: '2' (0 or 1)"),
                                       (dict(cog="yes"), "bad value for cog"),
                                       (dict(overview_resampling="cubic"),
                                        "bad value for overview_resampling: 'cubic' (nearest or average)"),
                                       (dict(cog="1", gpu_deflate="0"), "gpu_deflate=0")])
def test_config_refuses(tmp_path, extra, msg):
    with pytest.raises(host.HostError, match=msg.replace("(", r"\(").replace(")", r"\)")):
        host.parse_config(_config(tmp_path, **extra))


def _gcn10(args, cwd):
    exe = os.path.join(ROOT, "bin", "gcn10")
    return subprocess.run([exe] + args, cwd=cwd, capture_output=True, text=True, timeout=120)


def test_cli_help_lists_cog():
    p = _gcn10(["-h"], ROOT)
    assert p.returncode == 0
    assert "--cog" in p.stdout and "--overview-resampling" in p.stdout


@pytest.mark.parametrize("cfg_extra,args,msg", [
    (dict(cog="3"), [], "bad value for cog"),
    (dict(overview_resampling="mode"), [], "bad value for overview_resampling"),
    (dict(cog="1", gpu_deflate="0"), [], "gpu_deflate=0"),
    (dict(gpu_deflate="0"), ["--cog"], "gpu_deflate=0"),
    ({}, ["--cog", "--overview-resampling", "bilinear"], "bad value for overview_resampling"),
])
def test_cli_refuses_before_any_gpu(tmp_path, cfg_extra, args, msg):
    cfg = _config(tmp_path, log_dir=str(tmp_path / "logs"), **cfg_extra)
    p = _gcn10(["-c", cfg] + args, str(tmp_path))
    assert p.returncode == 1, p.stdout + p.stderr
    assert msg in p.stderr
    assert "no CPU fallback" not in p.stderr        # refused at config load, not when the GPU is sought
