"""GPU tile LZW (include/gcn10_gpu.h, gcn10_gpu_lzw_strip) and the compress=lzw runs of the gcn10 program.

Every stream is decoded by the strict TIFF 6.0 section 13 decoder below and compared with its zero-padded tile;
the same streams, wrapped as one-tile TIFFs, decode alike through libtiff (PIL) and the host reader."""
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

from oracle import cn_oracle_c as oc
from tests import tiffutil
from tests.conftest import LOOKUPS, ROOT
from tests.util import ESA_NASTY, HSG_NASTY

pytestmark = pytest.mark.gpu

CN_VALUES = np.array([0, 15, 30, 35, 41, 48, 51, 55, 59, 62, 68, 72, 77, 83, 98, 255], dtype=np.uint8)
CLEAR, EOI = 256, 257


class LzwError(ValueError):
    pass


def strict_lzw_decode(stream, expect_len):
    """TIFF LZW as libtiff reads it (MSB-first, 9..12-bit codes, early change), strictly: the stream must start
    with ClearCode, no code may need 13 bits or lie above the next free code, and it must end with EOI.
    Returns (bytes, statistics)."""
    d = bytes(stream) + b"\0\0\0"
    total = len(stream) * 8
    pos, width, nxt, prev = 0, 9, 258, None
    table = [bytes([i]) for i in range(256)] + [b"", b""]
    out = bytearray()
    stats = {"clears": 0, "max_width": 9, "codes": 0}
    first = True
    while True:
        if pos + width > total:
            raise LzwError("stream ends without EOI")
        i = pos >> 3
        v = (d[i] << 16 | d[i + 1] << 8 | d[i + 2]) >> (24 - (pos & 7) - width) & ((1 << width) - 1)
        pos += width
        if first and v != CLEAR:
            raise LzwError("stream does not start with ClearCode")
        first = False
        if v == EOI:
            break
        if v == CLEAR:
            stats["clears"] += 1
            del table[258:]
            width, nxt, prev = 9, 258, None
            continue
        stats["codes"] += 1
        if prev is None:
            if v > 255:
                raise LzwError("first code after ClearCode is not a literal")
            s = table[v]
        else:
            if v > nxt:
                raise LzwError("code %d above the next free code %d" % (v, nxt))
            s = table[v] if v < nxt else table[prev] + table[prev][:1]
            table.append(table[prev] + s[:1])
            nxt += 1
            if nxt + 1 >= (1 << width):
                width += 1
                if width > 12:
                    raise LzwError("a 13-bit code would be needed")
                stats["max_width"] = max(stats["max_width"], width)
        out += s
        prev = v
    if len(out) != expect_len:
        raise LzwError("decoded %d bytes, expected %d" % (len(out), expect_len))
    return bytes(out), stats


def _tile(img, ty, tx):
    want = np.zeros((256, 256), np.uint8)
    part = img[ty * 256:(ty + 1) * 256, tx * 256:(tx + 1) * 256]
    want[:part.shape[0], :part.shape[1]] = part
    return want


def _encode(engine, rasters, W, H, **kw):
    bufs = [engine.upload(np.ascontiguousarray(r)) for r in rasters]
    try:
        return engine.lzw_strip([b.ptr for b in bufs], W, H, **kw)
    finally:
        for b in bufs:
            b.close()


def _check(engine, rasters, W, H):
    """Every stream decodes strictly to its tile; returns (total stream bytes, statistics of every stream)."""
    data, table, used = _encode(engine, rasters, W, H)
    across, down = (W + 255) // 256, (H + 255) // 256
    assert table.shape == (len(rasters), down, across, 2)
    bound = engine.lzw_arena_bound(W, H, len(rasters))
    assert used <= bound
    total, stats = 0, []
    for r, img in enumerate(rasters):
        for ty in range(down):
            for tx in range(across):
                off, size = int(table[r, ty, tx, 0]), int(table[r, ty, tx, 1])
                assert off != 0xFFFFFFFF and off % 16 == 0 and 0 < size <= 82032 and off + size <= used
                got, st = strict_lzw_decode(data[off:off + size], 65536)
                assert got == _tile(img, ty, tx).tobytes(), (r, ty, tx)
                total += size
                stats.append(st)
    return total, stats


def _rasters(kind, H, W, seed):
    rng = np.random.default_rng(seed)
    if kind == "zeros":
        return np.zeros((H, W), np.uint8)
    if kind == "constant":
        return np.full((H, W), 77, np.uint8)
    if kind == "nodata":
        return np.full((H, W), 255, np.uint8)
    if kind == "patches":               # 25-px soil cells x landcover patches, like a CN raster
        a = rng.choice(CN_VALUES, size=((H + 24) // 25, (W + 24) // 25))
        return np.repeat(np.repeat(a, 25, axis=0), 25, axis=1)[:H, :W].copy()
    if kind == "noisy":                 # i.i.d. over the CN value set
        return rng.choice(CN_VALUES, size=(H, W)).astype(np.uint8)
    if kind == "iid":                   # i.i.d. bytes: fill the dictionary, force clears inside segments
        return rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["zeros", "constant", "nodata", "patches", "noisy", "iid"])
def test_streams_decode_strictly_to_the_tiles(engine, kind):
    W, H = 768, 512
    _, stats = _check(engine, [_rasters(kind, H, W, 3)], W, H)
    if kind == "iid":
        # the dictionary fills (codes reach 10 bits) and is cleared inside the tile, beyond the segment clears
        assert all(s["max_width"] == 10 and s["clears"] > 4 for s in stats)


def _de_bruijn_pairs():
    """A byte sequence of 65536 + 1 bytes in which no pair of consecutive bytes repeats (de Bruijn, order 2):
    every byte of it costs the encoder one code and one dictionary entry."""
    seq, a = [], [0] * 3

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, 256):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return np.array(seq + seq[:1], np.uint8)


def test_code_width_boundaries_are_crossed_exactly(engine):
    """A segment that starts with n pair-distinct bytes and ends in a run assigns one entry per byte of the first
    part: n swept across 253 (next code 511: codes become 10 bits), 765 (next code 1023: this encoder clears the
    dictionary) and 1789 (next code 2047, which this encoder never reaches: it must clear before) puts every
    crossing at seven consecutive positions; every tile decodes strictly and no code is wider than 10 bits."""
    db = _de_bruijn_pairs()
    tiles = []
    for centre in (253, 765, 1789):
        for n in range(centre - 3, centre + 4):
            t = np.full(65536, 30, np.uint8)
            for s in range(4):                          # every segment of the tile, at a different offset
                t[s * 16384:s * 16384 + n] = db[s * 5000:s * 5000 + n]
            tiles.append(t.reshape(256, 256))
    img = np.concatenate(tiles, axis=1)
    _, stats = _check(engine, [img], img.shape[1], 256)
    assert all(st["max_width"] == 10 for st in stats)
    # a segment that is nothing but pair-distinct bytes ends on a full dictionary's clear
    img = db[:65536].reshape(256, 256)
    _, stats = _check(engine, [img], 256, 256)
    assert stats[0]["clears"] >= 4 + 4 * 21


@pytest.mark.parametrize("n_rasters", [1, 18])
def test_edge_tiles_and_raster_counts(engine, n_rasters):
    """W = 36001 (a 1-pixel column of edge tiles) and rows not a multiple of 256, one raster; 18 rasters of
    every kind in one launch."""
    if n_rasters == 1:
        W, H = 36001, 300
        rasters = [_rasters("patches", H, W, 4)]
    else:
        kinds = ["patches", "noisy", "zeros", "iid", "constant", "nodata"]
        W, H = 600, 300
        rasters = [_rasters(kinds[r % len(kinds)], H, W, 10 + r) for r in range(n_rasters)]
    _check(engine, rasters, W, H)


def test_arena_one_byte_too_small(engine):
    """The stream that does not fit gets offset 0xffffffff and size 0; the others are where a full arena has
    them; nothing is written behind arena_cap (guard bytes)."""
    from gcn10_amd import gpu
    W, H = 512, 512
    rasters = [_rasters("noisy", H, W, 7), _rasters("patches", H, W, 8)]
    full_data, full_tab, used = _encode(engine, rasters, W, H)
    ft = full_tab.reshape(-1, 2)
    last = int(np.argmax(ft[:, 0]))
    cap = int(ft[last, 0]) + (int(ft[last, 1]) + 15) // 16 * 16 - 1
    guard = 4096
    bufs = [engine.upload(r) for r in rasters]
    ptrs = engine.upload(np.array([b.ptr for b in bufs], np.uint64))
    arena = engine.upload(np.full(cap + guard + 15, 0xA5, np.uint8))
    table, cursor = engine.alloc(ft.size * 4), engine.alloc(8)
    try:
        engine._chk(gpu.lib().gcn10_gpu_lzw_strip(engine._ctx, ptrs.ptr, 2, W, H, arena.ptr, cap, table.ptr,
                                                  cursor.ptr, None), "gcn10_gpu_lzw_strip")
        tab = engine.download(table.ptr, ft.shape, dtype=np.uint32)
        after = engine.download(arena.ptr, (cap + guard + 15,))
    finally:
        for b in bufs + [ptrs, arena, table, cursor]:
            b.close()
    assert tab[last, 0] == 0xFFFFFFFF and tab[last, 1] == 0
    keep = np.arange(len(ft)) != last
    assert np.array_equal(tab[keep], ft[keep])
    assert (after[cap:] == 0xA5).all()
    for off, size in tab[keep]:
        assert np.array_equal(after[off:off + size], full_data[off:off + size])


def _one_tile_tiff(path, stream, monkeypatch):
    with monkeypatch.context() as m:
        m.setattr(tiffutil, "lzw_encode", lambda raw: bytes(stream))
        tiffutil.write_tiff(str(path), np.zeros((256, 256), np.uint8), compression=5, tile=(256, 256))


def _pil_lzw_bytes(tile):
    f = io.BytesIO()
    Image.fromarray(tile).save(f, format="TIFF", compression="tiff_lzw")
    return int(Image.open(io.BytesIO(f.getvalue())).tag_v2[279][0])


def test_libtiff_and_the_host_reader_decode_the_streams_alike(engine, tmp_path, monkeypatch):
    from gcn10_amd import host
    W, H = 1024, 512
    rasters = [_rasters(k, H, W, 30 + i) for i, k in enumerate(("patches", "noisy", "zeros", "iid"))]
    data, table, _ = _encode(engine, rasters, W, H)
    for r, img in enumerate(rasters):
        for ty in range(2):
            for tx in range(4):
                off, size = int(table[r, ty, tx, 0]), int(table[r, ty, tx, 1])
                p = tmp_path / ("t%d_%d_%d.tif" % (r, ty, tx))
                _one_tile_tiff(p, data[off:off + size], monkeypatch)
                want = _tile(img, ty, tx)
                im = Image.open(str(p))
                assert im.tag_v2[259] == 5
                assert np.array_equal(np.array(im), want), ("libtiff", r, ty, tx)
                with host.Raster(str(p)) as hr:
                    assert np.array_equal(hr.read(0, 0, 256, 256), want), ("host reader", r, ty, tx)


def test_segmenting_keeps_the_compression_of_libtiff(engine):
    """Over patchy and noisy tiles the streams total at most 1.15x the bytes of libtiff's own LZW of the same
    tiles (each its own one-strip image)."""
    W, H = 1024, 512
    ours = theirs = 0
    for kind, seed in (("patches", 40), ("noisy", 41)):
        img = _rasters(kind, H, W, seed)
        got, _ = _check(engine, [img], W, H)
        ours += got
        theirs += sum(_pil_lzw_bytes(_tile(img, ty, tx)) for ty in range(2) for tx in range(4))
    assert ours <= 1.15 * theirs, (ours, theirs, ours / theirs)


# ---- the gcn10 program with compress=lzw (after tests/test_cli.py) --------------------------------

GCN10 = os.path.join(ROOT, "bin", "gcn10")
CONDS, HCS, ARCS = ("drained", "undrained"), ("p", "f", "g"), ("i", "ii", "iii")
ESA_GT = [10.0, 0.001, 0.0, 50.0, 0.0, -0.001]
SOIL_GT = [9.9875, 0.025, 0.0, 50.0125, 0.0, -0.025]
BLOCKS = [(101, 10.0, 49.0, 11.0, 50.0),
          (102, 11.0, 48.0, 12.0, 49.0),
          (103, 12.5, 47.5, 13.5, 48.5),
          (104, 20.0, 20.0, 21.0, 21.0)]


def _world(tmp_path, seed=5, extra_cfg=""):
    rng = np.random.default_rng(seed)
    small = rng.choice(ESA_NASTY, size=(2000 // 20, 3000 // 20))
    esa = np.repeat(np.repeat(small, 20, axis=0), 20, axis=1)
    noise = rng.integers(0, 256, size=esa.shape, dtype=np.uint8)
    esa = np.where(noise < 30, rng.choice(ESA_NASTY, size=esa.shape), esa).astype(np.uint8)
    soil = rng.choice(HSG_NASTY, size=(2000 // 25 + 2, 3000 // 25 + 2)).astype(np.uint8)
    tiffutil.write_tiff(str(tmp_path / "esa.tif"), esa, gt=ESA_GT, compression=8, tile=(512, 512))
    tiffutil.write_tiff(str(tmp_path / "soil_lzw.tif"), soil, gt=SOIL_GT, compression=5, rows_per_strip=8)
    tiffutil.write_block_shapefile(str(tmp_path / "blocks"), BLOCKS)
    (tmp_path / "config.txt").write_text(
        "# test config\nhysogs_data_path=%s\nesa_data_path=%s\nblocks_shp_path=%s\n"
        "lookup_table_path=%s\nlog_dir=%s\nstrip_rows=256\nio_threads=4\nworkers_per_gpu=1\n%s"
        % (tmp_path / "soil_lzw.tif", tmp_path / "esa.tif", tmp_path / "blocks.shp", LOOKUPS, tmp_path / "logs",
           extra_cfg))
    return esa, soil


def _run(tmp_path, *args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([GCN10, *args], cwd=str(tmp_path), capture_output=True, text=True, env=e, timeout=600)


def _check_outputs(tmp_path, esa, soil, tables, blocks, cond_mask=3, table_mask=0x1FF):
    for bid, *bbox in blocks:
        xo, yo, W, H, gt = oc.window(ESA_GT, 3000, 2000, bbox)
        sxo, syo, hsx, hsy, sgt = oc.window(SOIL_GT, soil.shape[1], soil.shape[0], bbox)
        want = oc.process_block_mem(esa[yo:yo + H, xo:xo + W], gt, soil[syo:syo + hsy, sxo:sxo + hsx], sgt,
                                    tables, cond_mask=cond_mask, table_mask=table_mask)
        for c, cond in enumerate(CONDS):
            for k in range(9):
                if not (cond_mask >> c) & 1 or not (table_mask >> k) & 1:
                    continue
                p = tmp_path / ("cn_rasters_%s" % cond) / ("cn_%s_%s_%d.tif" % (HCS[k // 3], ARCS[k % 3], bid))
                im = Image.open(str(p))
                assert np.array_equal(np.array(im), want[c * 9 + k]), p
                t = im.tag_v2
                assert t[259] == 5 and 317 not in t and t[322] == 256 and t[323] == 256, p
                assert tuple(t[33550]) == (gt[1], -gt[5], 0.0)


@pytest.mark.parametrize("gpu_deflate", [2, 1], ids=["gpu_deflate-2", "gpu_deflate-1"])
def test_lzw_run_equals_oracle(tmp_path, tables, gpu_deflate):
    esa, soil = _world(tmp_path, extra_cfg="gpu_deflate=%d\ncompress=LZW\n" % gpu_deflate)
    (tmp_path / "ids.txt").write_text("101 102\n103\n104\n")
    out = _run(tmp_path, "-c", "config.txt", "-l", "ids.txt")
    assert out.returncode == 0, out.stderr[-2000:]
    log = (tmp_path / "logs" / "rank_0.log").read_text()
    assert "processed 4 blocks on 1 ranks" in log and ", gpu lzw" in log
    _check_outputs(tmp_path, esa, soil, tables, BLOCKS[:3])


def test_lzw_single_lookup_from_flags(tmp_path, tables):
    esa, soil = _world(tmp_path)
    (tmp_path / "ids.txt").write_text("101 103\n")
    out = _run(tmp_path, "-c", "config.txt", "-l", "ids.txt", "--lookups", "g_ii", "--conditions", "drained",
               "--compress", "lzw")
    assert out.returncode == 0, out.stderr[-2000:]
    assert sorted(os.listdir(tmp_path / "cn_rasters_drained")) == ["cn_g_ii_101.tif", "cn_g_ii_103.tif"]
    assert not (tmp_path / "cn_rasters_undrained").exists()
    _check_outputs(tmp_path, esa, soil, tables, (BLOCKS[0], BLOCKS[2]), cond_mask=1, table_mask=1 << 7)


def test_lzw_direct_io_through_the_spill_path(tmp_path, tables):
    esa, soil = _world(tmp_path, seed=11, extra_cfg="compress=lzw\ndirect_io=1\n")
    (tmp_path / "ids.txt").write_text("101 103\n")
    out = _run(tmp_path, "-c", "config.txt", "-l", "ids.txt", env={"GCN10_PINNED_ARENA_BYTES": "4096"})
    assert out.returncode == 0, out.stderr[-2000:]
    _check_outputs(tmp_path, esa, soil, tables, (BLOCKS[0], BLOCKS[2]))


def test_lzw_full_size_block_of_the_real_vrt_shape(tmp_path, tables):
    """36001 x 36001 (1-pixel edge tiles, rows not 16-byte aligned), three rasters checked on 600 rows."""
    import bench
    Image.MAX_IMAGE_PIXELS = None
    size, px = 36001, 8.3333333333330430e-05
    esa, _, coarse, _ = bench.synth_block(5, size, "patches")
    hs = coarse.shape[0]
    egt = [0.0, px, 0.0, 3.0, 0.0, -px]
    sgt = [0.0, 3.0 / hs, 0.0, 3.0, 0.0, -3.0 / hs]
    tiffutil.write_tiff(str(tmp_path / "esa.tif"), esa, gt=egt, compression=8, tile=(1024, 1024))
    tiffutil.write_tiff(str(tmp_path / "soil.tif"), coarse, gt=sgt, compression=5, rows_per_strip=16)
    tiffutil.write_block_shapefile(str(tmp_path / "blocks"), [(1, 0.0, 0.0, 3.0, 3.0)])
    (tmp_path / "config.txt").write_text(
        "hysogs_data_path=%s\nesa_data_path=%s\nblocks_shp_path=%s\nlookup_table_path=%s\nlog_dir=%s\ncompress=lzw\n"
        % (tmp_path / "soil.tif", tmp_path / "esa.tif", tmp_path / "blocks.shp", LOOKUPS, tmp_path / "logs"))
    out = _run(tmp_path, "-c", "config.txt")
    assert out.returncode == 0, out.stderr[-2000:]
    xo, yo, W, H, gt = oc.window(egt, size, size, [0.0, 0.0, 3.0, 3.0])
    assert (W, H) == (size, size)
    sxo, syo, hsx, hsy, sg = oc.window(sgt, hs, hs, [0.0, 0.0, 3.0, 3.0])
    y0 = 20000
    want = oc.process_block_mem(esa[yo + y0:yo + y0 + 600, xo:xo + W], [gt[0], gt[1], 0.0, gt[3] + y0 * gt[5], 0.0, gt[5]],
                                coarse[syo:syo + hsy, sxo:sxo + hsx], sg, tables)
    for r in (0, 13, 17):
        c, k = divmod(r, 9)
        p = tmp_path / ("cn_rasters_%s" % CONDS[c]) / ("cn_%s_%s_1.tif" % (HCS[k // 3], ARCS[k % 3]))
        im = Image.open(str(p))
        assert im.tag_v2[259] == 5
        a = np.array(im)
        assert a.shape == (size, size)
        assert np.array_equal(a[y0:y0 + 600], want[r]), p
