"""CPU: the GeoTIFF writer with O_DIRECT on (config key direct_io).  Only gcn10_tiff_put_extent aligns its
writes; a put_tile or put_tiles goes at any position and length, which ext4 and xfs refuse on an O_DIRECT
descriptor (EINVAL).  The writer must then write that file buffered instead of failing it, and the file must
come out as the same puts would make it without direct I/O."""
import os
import zlib

import numpy as np
import pytest
from PIL import Image

from gcn10_amd import host
from tests.test_cog_writer import GT, level_image, pil_levels, tile_of
from tests.tiffutil import lzw_encode

O_DIRECT = getattr(os, "O_DIRECT", 0)
pytestmark = pytest.mark.skipif(not O_DIRECT, reason="no O_DIRECT on this platform")


def unaligned_direct_write_refused(directory) -> bool:
    """Whether the file system under `directory` refuses an unaligned write on an O_DIRECT descriptor."""
    path = os.path.join(str(directory), "probe.bin")
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | O_DIRECT, 0o644)
    try:
        os.pwrite(fd, b"x" * 100, 1)
        return False
    except OSError as e:
        assert e.errno == 22, e                 # EINVAL, nothing else
        return True
    finally:
        os.close(fd)
        os.unlink(path)


def part_is_direct(path) -> bool:
    """O_DIRECT on this process's descriptor of `path`.part (the file being written), from /proc/self/fdinfo."""
    want = os.path.realpath(path + ".part")
    for fd in os.listdir("/proc/self/fd"):
        try:
            if os.readlink("/proc/self/fd/" + fd) != want:
                continue
            with open("/proc/self/fdinfo/" + fd) as f:
                flags = next(int(line.split()[1], 8) for line in f if line.startswith("flags:"))
        except OSError:
            continue
        return bool(flags & O_DIRECT)
    raise AssertionError("no descriptor of %s.part is open" % path)


@pytest.fixture(scope="module")
def refused(tmp_path_factory):
    r = unaligned_direct_write_refused(tmp_path_factory.mktemp("probe"))
    print("file system refuses unaligned O_DIRECT writes: %s" % r)
    return r


def write(path, W, H, pattern, direct, cog, compression=8, seed=0, refused=True):
    """Writes a plain file (cog=False) or a COG of W x H by one pattern of puts; returns the images per level.
    pattern: "tile" (put_tile only), "tiles" (put_tiles, one call per tile row), or "mixed" (put_extent first,
    then put_tile, put_extent and put_tiles by turns, row by row).  With direct=True: where the file system refuses
    unaligned O_DIRECT writes (`refused`), direct I/O must really be on up to the first unaligned put; after that
    put, and on any file system, the descriptor must be buffered."""
    L = host.cog_levels(W, H) if cog else 0
    enc = (lambda b: zlib.compress(b, 1)) if compression == 8 else lzw_encode
    wr = host.TiffWriter(path, W, H, GT, n_levels=L if cog else None, compression=compression, direct=direct)
    imgs, n, fell_back = {}, 0, False
    try:
        if direct:
            assert part_is_direct(path) == wr.direct
            assert wr.direct or not refused, "direct I/O was not on to begin with"
        for k in range(L, -1, -1):
            imgs[k] = img = level_image(W, H, k, seed)
            across, down = wr.tiles(k)
            for ty in range(down):
                row = [(tx, ty, enc(tile_of(img, tx, ty))) for tx in range(across)]
                kind = {"tile": "tile", "tiles": "tiles", "mixed": ("extent", "tile", "extent", "tiles")[n % 4]}[pattern]
                if direct and not fell_back:
                    # nothing unaligned was written yet: direct I/O is still on (extents are aligned)
                    assert part_is_direct(path) == wr.direct, (pattern, k, ty)
                if kind == "tile":
                    for tx, _ty, d in row:
                        assert wr.put_tile(tx, ty, d, level=k) == 0, (pattern, k, tx, ty)
                elif kind == "tiles":
                    assert wr.put_tiles(row, level=k) == 0, (pattern, k, ty)
                else:
                    assert wr.put_extent(row, level=k) == 0, (pattern, k, ty)
                if direct and kind != "extent":
                    # never an unaligned write on an O_DIRECT descriptor: this file is buffered from here on
                    assert not part_is_direct(path), (pattern, k, ty)
                    fell_back = True
                n += 1
        wr.finish()
    except BaseException:
        wr.abort()
        raise
    return L, imgs


PATTERNS = ["tile", "tiles", "mixed"]
SHAPES = [(300, 513), (1040, 300)]


@pytest.mark.parametrize("cog", [False, True], ids=["plain", "cog"])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("W,H", SHAPES)
def test_direct_puts_decode_to_their_input(tmp_path, refused, W, H, pattern, cog):
    path = str(tmp_path / "d.tif")
    L, imgs = write(path, W, H, pattern, True, cog, seed=W, refused=refused)
    assert os.path.exists(path) and not os.path.exists(path + ".part")
    levels = pil_levels(path)
    assert len(levels) == L + 1
    for k in range(L + 1):
        np.testing.assert_array_equal(levels[k], imgs[k], err_msg="%s level %d" % (pattern, k))
    with host.Raster(path) as r:
        np.testing.assert_array_equal(r.read(0, 0, W, H), imgs[0])
    if cog:
        from tests import cogcheck
        cogcheck.check_cog(path, n_levels=L)


@pytest.mark.parametrize("cog", [False, True], ids=["plain", "cog"])
@pytest.mark.parametrize("pattern", ["tile", "tiles"])
def test_unaligned_puts_make_the_buffered_file(tmp_path, refused, pattern, cog):
    """Without put_extent nothing is aligned, so the direct file is the buffered one byte for byte: same offsets,
    same append position, same COG order."""
    a, b = str(tmp_path / "direct.tif"), str(tmp_path / "buffered.tif")
    write(a, 700, 513, pattern, True, cog, compression=5, seed=4, refused=refused)
    write(b, 700, 513, pattern, False, cog, compression=5, seed=4)
    assert open(a, "rb").read() == open(b, "rb").read()


def test_put_tiles_matches_put_tile(tmp_path):
    """put_tiles is n put_tile calls in one (gathered writes), also past the 512 buffers of one system call."""
    W, H = 256 * 600, 256
    img = (np.arange(W, dtype=np.uint32)[None, :] * 7 + np.arange(H, dtype=np.uint32)[:, None] * 3).astype(np.uint8)
    tiles = [(tx, 0, zlib.compress(tile_of(img, tx, 0), 1)) for tx in range(W // 256)]
    a, b = str(tmp_path / "a.tif"), str(tmp_path / "b.tif")
    wa, wb = host.TiffWriter(a, W, H, GT), host.TiffWriter(b, W, H, GT)
    assert wa.put_tiles(tiles) == 0
    for tx, ty, d in tiles:
        assert wb.put_tile(tx, ty, d) == 0
    wa.finish()
    wb.finish()
    assert open(a, "rb").read() == open(b, "rb").read()
    with Image.open(a) as im:
        np.testing.assert_array_equal(np.array(im), img)


def test_direct_extents_stay_direct(tmp_path, refused):
    """put_extent alone keeps O_DIRECT on to the end: the fallback is for unaligned puts only."""
    path = str(tmp_path / "e.tif")
    img = level_image(1040, 600, 0, 9)
    wr = host.TiffWriter(path, 1040, 600, GT, direct=True)
    try:
        assert wr.direct or not refused
        for ty in range(3):
            assert wr.put_extent([(tx, ty, zlib.compress(tile_of(img, tx, ty), 1)) for tx in range(5)]) == 0
            assert part_is_direct(path) == wr.direct
        wr.finish()
    except BaseException:
        wr.abort()
        raise
    with Image.open(path) as im:
        np.testing.assert_array_equal(np.array(im), img)
