"""CPU: what the GeoTIFF module (gcn10_amd/csrc/host/tiff_*.c) does at its edges, pinned before the module was split
by subject: every window of a tiny raster through the window reader and the read planner, what each of the three tile
puts does with each kind of refusal, and the outcome of opening hand-made files.  The expected tables were recorded
from the library as it stood before the split (profiles/tiff_split/pins_on_parent.txt).  One refusal is not here:
"no room below 4 GiB" takes 4 GiB of tile data to reach, in this test as in the sanitizer program; the three puts ask
one function for it (room_up_to in tiff_write.c), which is read, not run."""
import ctypes as C
import itertools
import os
import random
import struct
import zlib

import numpy as np
import pytest

from gcn10_amd import host
from tests import tiffutil
from tests.lzw_model import lzw_decode_ref

GT = [10.0, 0.5, 0.0, 50.0, 0.0, -0.5]
W, H = 13, 11
IMG = (np.arange(W * H, dtype=np.uint32).reshape(H, W) + 17).astype(np.uint8)      # 143 distinct values
assert len(set(IMG.reshape(-1).tolist())) == W * H

# struct gcn10_chunk_ref as numpy sees it (host._ChunkRef: an int, 4 bytes of padding, a uint64, eleven uint32)
_U32 = ["nbytes", "chunk_w", "rows", "src_x", "src_y", "copy_w", "copy_h", "dst_x", "dst_y", "flags", "out_len"]
CHUNK = np.dtype({"names": ["fd", "file_off"] + _U32, "formats": ["<i4", "<u8"] + ["<u4"] * 11,
                  "offsets": [0, 8] + [16 + 4 * i for i in range(11)], "itemsize": C.sizeof(host._ChunkRef)})
assert CHUNK.itemsize == 64


class Tiff:
    """One directory of a TIFF file through the module's own entry points (host_internal.h)."""

    def __init__(self, path, level=0):
        L = host.lib()
        L.gcn10_tiff_open_reader_ifd.restype = C.c_void_p
        L.gcn10_tiff_open_reader_ifd.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
        L.gcn10_tiff_close_reader.argtypes = [C.c_void_p]
        L.gcn10_tiff_close_reader.restype = None
        L.gcn10_tiff_reader_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double)]
        L.gcn10_tiff_reader_info.restype = None
        L.gcn10_tiff_read_window.restype = C.c_int
        L.gcn10_tiff_read_window.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                             C.c_char_p, C.c_size_t]
        L.gcn10_tiff_plan_window.restype = C.c_int
        L.gcn10_tiff_plan_window.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint,
                                             C.POINTER(host._ReadPlan), C.c_char_p, C.c_size_t]
        L.gcn10_read_plan_free.argtypes = [C.POINTER(host._ReadPlan)]
        L.gcn10_read_plan_free.restype = None
        self.L, self.err, self.why = L, C.create_string_buffer(1024), C.c_int(-7)
        self.h = L.gcn10_tiff_open_reader_ifd(os.fsencode(path), level, C.byref(self.why), self.err, 1024)
        self.buf = np.zeros(1 << 16, np.uint8)

    def message(self):
        return self.err.value.decode(errors="replace")

    def info(self):
        xs, ys, gt = C.c_int(), C.c_int(), (C.c_double * 6)()
        self.L.gcn10_tiff_reader_info(self.h, C.byref(xs), C.byref(ys), gt)
        return xs.value, ys.value, list(gt)

    def read(self, x, y, w, h):
        """(rc, pixels or None)"""
        if w * h > self.buf.size:
            self.buf = np.zeros(w * h, np.uint8)
        self.buf[:max(w * h, 0)] = 0xEE
        rc = self.L.gcn10_tiff_read_window(self.h, x, y, w, h, self.buf.ctypes.data, max(w, 0), self.err, 1024)
        return rc, (self.buf[:w * h].reshape(h, w) if rc == 0 else None)

    def plan(self, x, y, w, h, codecs=7):
        """(rc, chunks as a CHUNK array, covered, max_chunk_bytes, staged_bytes)"""
        plan = host._ReadPlan()
        rc = self.L.gcn10_tiff_plan_window(self.h, x, y, w, h, 0, 0, codecs, C.byref(plan), self.err, 1024)
        n = plan.n if rc == 0 else 0
        chunks = np.frombuffer(C.string_at(plan.chunks, n * CHUNK.itemsize), CHUNK).copy() if n else np.zeros(0, CHUNK)
        out = rc, chunks, plan.covered, plan.max_chunk_bytes, plan.staged_bytes
        self.L.gcn10_read_plan_free(C.byref(plan))
        return out

    def close(self):
        if self.h:
            self.L.gcn10_tiff_close_reader(self.h)
            self.h = None


# ---- 1. every window of a tiny raster ---------------------------------------------------------------------------

SHAPES = {"tiles4x3": dict(tile=(4, 3)), "tiles16": dict(tile=(16, 16)), "strips3": dict(rows_per_strip=3),
          "strips11": dict(rows_per_strip=11)}
CODECS = {"none": dict(compression=1), "lzw": dict(compression=5), "lzw_p2": dict(compression=5, predictor=2),
          "deflate": dict(compression=8), "deflate_p2": dict(compression=8, predictor=2),
          "packbits": dict(compression=32773)}
ALL_WINDOWS = [(x, y, w, h) for y in range(H) for h in range(1, H - y + 1) for x in range(W)
               for w in range(1, W - x + 1)]
assert len(ALL_WINDOWS) == 91 * 66
#: the shapes whose every window is checked; of the other two a fixed-seed sample of 600 windows plus the single-pixel,
#: edge and full windows
EVERY_WINDOW = ("tiles4x3", "strips3")
EDGE_WINDOWS = [(0, 0, W, H), (W - 1, H - 1, 1, 1), (0, 0, 1, 1), (W - 1, 0, 1, H), (0, H - 1, W, 1), (0, 0, 4, 3),
                (4, 3, 4, 3), (12, 9, 1, 2), (3, 2, 2, 2), (0, 9, W, 2), (8, 0, 5, H)]


def _decoded_chunk(data, c, cache):
    """The pixels a staged chunk stands for, chunk_w wide, as gcn10_gpu_inflate_tiles is asked to make them."""
    key = (int(c["file_off"]), int(c["nbytes"]), int(c["flags"]))
    if key not in cache:
        raw = data[key[0]:key[0] + key[1]]
        cw, flags = int(c["chunk_w"]), key[2]
        if flags & 1:                                           # GCN10_TILE_RAW: out_len bytes of pixels
            t = np.zeros(-(-len(raw) // cw) * cw, np.uint8)
            t[:len(raw)] = np.frombuffer(raw, np.uint8)
        elif flags & 4:                                         # GCN10_TILE_LZW
            t = np.frombuffer(lzw_decode_ref(raw, cw * int(c["rows"])), np.uint8)
        else:
            t = np.frombuffer(zlib.decompress(raw), np.uint8)[:cw * int(c["rows"])]
        t = t.reshape(-1, cw)
        if flags & 2:                                           # GCN10_TILE_PREDICTOR2
            t = np.cumsum(t, axis=1, dtype=np.uint64).astype(np.uint8)
        cache[key] = t
    return cache[key]


@pytest.mark.parametrize("codec", list(CODECS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_window_reads_and_plans_as_the_numpy_slice(tmp_path, shape, codec):
    p = str(tmp_path / "t.tif")
    tiffutil.write_tiff(p, IMG, gt=GT, **SHAPES[shape], **CODECS[codec])
    data = open(p, "rb").read()
    windows = ALL_WINDOWS if shape in EVERY_WINDOW else \
        EDGE_WINDOWS + random.Random(20).sample(ALL_WINDOWS, 600)
    t = Tiff(p)
    assert t.h, t.message()
    cache, painted = {}, np.zeros((H, W), np.int32)
    want_flags = {"none": 1, "lzw": 4, "lzw_p2": 6, "deflate": 0, "deflate_p2": 2}.get(codec)
    try:
        for (x, y, w, h) in windows:
            rc, got = t.read(x, y, w, h)
            assert rc == 0 and np.array_equal(got, IMG[y:y + h, x:x + w]), (x, y, w, h)
            rc, ch, covered, max_bytes, staged = t.plan(x, y, w, h)
            if codec == "packbits":
                assert rc == 1                                  # stays with the host reader
                continue
            assert rc == 0 and covered == w * h and staged == int(ch["nbytes"].sum()), (x, y, w, h)
            assert (ch["flags"] == want_flags).all() and (ch["nbytes"] > 0).all()
            assert (ch["file_off"] + ch["nbytes"] <= len(data)).all()
            assert (ch["src_x"] + ch["copy_w"] <= ch["chunk_w"]).all() and (ch["src_y"] + ch["copy_h"] <= ch["rows"]).all()
            assert ((ch["src_y"] + ch["copy_h"] - 1) * ch["chunk_w"] + ch["src_x"] + ch["copy_w"] <= ch["out_len"]).all()
            assert (ch["dst_x"] + ch["copy_w"] <= w).all() and (ch["dst_y"] + ch["copy_h"] <= h).all()
            if codec == "none":
                assert max_bytes == 0 and (ch["out_len"] == ch["nbytes"]).all()
            else:
                assert (ch["out_len"] == ch["chunk_w"] * ch["rows"]).all() and max_bytes == int(ch["out_len"].max())
            out, cnt = np.zeros((h, w), np.uint8), painted[:h, :w]
            cnt[:] = 0
            for c in ch:
                sx, sy, cw_, chh, dx, dy = (int(c[k]) for k in ("src_x", "src_y", "copy_w", "copy_h", "dst_x", "dst_y"))
                out[dy:dy + chh, dx:dx + cw_] = _decoded_chunk(data, c, cache)[sy:sy + chh, sx:sx + cw_]
                cnt[dy:dy + chh, dx:dx + cw_] += 1
            assert (cnt == 1).all(), (x, y, w, h)               # the rectangles tile the window: no gap, no overlap
            assert np.array_equal(out, IMG[y:y + h, x:x + w]), (x, y, w, h)
    finally:
        t.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_windows_one_pixel_outside_get_the_bounds_message_from_reader_and_planner(tmp_path, shape):
    p = str(tmp_path / "t.tif")
    tiffutil.write_tiff(p, IMG, gt=GT, compression=8, **SHAPES[shape])
    t = Tiff(p)
    try:
        for (x, y, w, h) in [(-1, 0, W, H), (0, -1, W, H), (1, 0, W, H), (0, 1, W, H), (W, 0, 1, 1), (0, H, 1, 1),
                             (0, 0, 0, 1), (0, 0, 1, 0), (W - 1, H - 1, 2, 1), (W - 1, H - 1, 1, 2)]:
            want = "window %d,%d %dx%d outside raster %dx%d" % (x, y, w, h, W, H)
            assert t.read(x, y, w, h)[0] == -1 and t.message() == want
            t.err.value = b""
            assert t.plan(x, y, w, h)[0] == -1 and t.message() == want
    finally:
        t.close()


# ---- 2. what the three puts do with a refusal -------------------------------------------------------------------

XS, YS = 600, 300               # 3 x 2 tiles; as a COG: level 1 = 300 x 150 (2 x 1), level 2 = 150 x 75 (1 x 1)
SIZES = {0: (3, 2), 1: (2, 1), 2: (1, 1)}


def _blob(level, tx, ty):
    return zlib.compress(bytes([1 + 10 * level + ty * 3 + tx]) * 65536, 1)


def _raw_put(w, kind, tiles, level=0, rel=None, extent_bytes=None):
    """tiles [(tx, ty, bytes)] through one call of put `kind`; for the extent put rel / extent_bytes override the
    back-to-back layout."""
    L, v = host.lib(), w._level(level)
    if kind == "tile":
        (tx, ty, d), = tiles
        return L.gcn10_tiff_put_tile(v, tx, ty, d, len(d))
    if kind == "tiles":
        return w.put_tiles(tiles, level)
    n = len(tiles)
    if rel is None:
        rel = list(itertools.accumulate([0] + [(len(d) + 15) & ~15 for _x, _y, d in tiles[:-1]]))
    size = max(r + len(d) for r, (_x, _y, d) in zip(rel, tiles))
    buf = np.zeros(size + 8192, np.uint8)
    for r, (_x, _y, d) in zip(rel, tiles):
        buf[r:r + len(d)] = np.frombuffer(d, np.uint8)
    arr = lambda t, vals: (t * n)(*vals)
    return L.gcn10_tiff_put_extent(v, buf.ctypes.data, size if extent_bytes is None else extent_bytes, n,
                                   arr(C.c_int, [t[0] for t in tiles]), arr(C.c_int, [t[1] for t in tiles]),
                                   arr(C.c_uint32, rel), arr(C.c_uint32, [len(t[2]) for t in tiles]))


def _fill(w, kind, level, skip=0):
    """Every tile of a level from tile index `skip` on, validly: True when every put was taken."""
    ax, dn = SIZES[level]
    tiles = [(i % ax, i // ax, _blob(level, i % ax, i // ax)) for i in range(skip, ax * dn)]
    if kind == "tile":
        return all([_raw_put(w, kind, [t], level) == 0 for t in tiles])
    return not tiles or _raw_put(w, kind, tiles, level) == 0


GOOD = _blob(0, 0, 0)
#: refusal -> (tiles of the refused call, keyword arguments of _raw_put)
REFUSALS = {
    "tx=-1": ([(-1, 0, GOOD)], {}),
    "ty=-1": ([(0, -1, GOOD)], {}),
    "tx=across": ([(3, 0, GOOD)], {}),
    "ty=down": ([(0, 2, GOOD)], {}),
    "nbytes=0": ([(0, 0, b"")], {}),
}


def _outcome(tmp_path, cog, kind, name, tiles, kw, before=0, level=0):
    """(return code of the refused put, whether the valid puts behind it were all taken, what finish said)"""
    p = str(tmp_path / "w.tif")
    w = host.TiffWriter(p, XS, YS, GT, n_levels=2 if cog else None)
    try:
        if cog:
            assert _fill(w, kind, 2) and _fill(w, kind, 1)
        if before:                                              # tiles 0 .. before-1 of level 0 go first
            for i in range(before):
                assert _raw_put(w, kind, [(i % 3, i // 3, _blob(0, i % 3, i // 3))]) == 0
        rc = _raw_put(w, kind, tiles, level, **kw)
        later = _fill(w, kind, 0, skip=before)
        try:
            w.finish()
        except host.HostError as e:
            return rc, later, str(e).replace(p, "<path>")
    finally:
        w.abort()
    for lv in range(3 if cog else 1):                           # every tile present, with its own pixels
        t = Tiff(p, lv)
        ax, dn = SIZES[lv]
        xs, ys, _gt = t.info()
        rcr, px = t.read(0, 0, xs, ys)
        assert rcr == 0
        for i in range(ax * dn):
            assert px[(i // ax) * 256, (i % ax) * 256] == 1 + 10 * lv + (i // ax) * 3 + (i % ax)
        t.close()
    return rc, later, "ok"


FAILED = "write error on <path>"
# recorded from the library before the split: (cog, put, refusal) -> outcome
TABLE = {}
for _cog in (False, True):
    for _name in REFUSALS:
        TABLE[(_cog, "tile", _name)] = (-1, True, "ok")         # a plain refusal: the writer stays usable
        TABLE[(_cog, "extent", _name)] = (-1, True, "ok")
        TABLE[(_cog, "tiles", _name)] = (-1, True, FAILED)     # the batch put marks the writer failed ...
# ... except where a COG's order rule sees the bad coordinate first (tile index -1 or below is "not above the last")
TABLE[(True, "tiles", "tx=-1")] = (-1, True, "ok")
TABLE[(True, "tiles", "ty=-1")] = (-1, True, "ok")


@pytest.mark.parametrize("cog,kind,name", sorted(TABLE), ids=lambda v: str(v))
def test_put_refusals_of_bad_tiles(tmp_path, cog, kind, name):
    tiles, kw = REFUSALS[name]
    assert _outcome(tmp_path, cog, kind, name, tiles, kw) == TABLE[(cog, kind, name)]


def test_put_tiles_refusal_at_position_0_and_in_the_second_batch(tmp_path):
    """A plain writer takes tiles in any order and more than once, so 514 tiles can go in one call: the bad one at
    position 0 stops before anything is written, the one at position 513 after the first batch of 512 went out.  Both
    mark the writer failed.  (A 3 x 2 COG cannot take 514 ascending tiles: its order rule refuses the call whole.)"""
    many = [(i % 3, (i // 3) % 2, _blob(0, i % 3, (i // 3) % 2)) for i in range(514)]
    for pos in (0, 513):
        for bad in ((-1, 0, GOOD), (3, 0, GOOD), (0, 2, GOOD), (0, 0, b"")):
            tiles = list(many)
            tiles[pos] = bad
            assert _outcome(tmp_path, False, "tiles", "", tiles, {}) == (-1, True, FAILED), (pos, bad[:2])
    assert _outcome(tmp_path, True, "tiles", "", many, {}) == (-1, True, "ok")
    # position 1 of a COG batch: the order rule passes (index 0, then 3 = tile (3, 0)), the coordinate check fails
    assert _outcome(tmp_path, True, "tiles", "", [(0, 0, GOOD), (3, 0, GOOD)], {}) == (-1, True, FAILED)


@pytest.mark.parametrize("cog", [False, True])
def test_put_extent_refusals_of_a_bad_layout(tmp_path, cog):
    two = [(0, 0, _blob(0, 0, 0)), (1, 0, _blob(0, 1, 0))]
    n0, n1 = len(two[0][2]), len(two[1][2])
    # stream 1 reaches beyond the extent: a plain refusal
    assert _outcome(tmp_path, cog, "extent", "", two, dict(rel=[0, 128], extent_bytes=128 + n1 - 1)) == (-1, True, "ok")
    # rel_off not increasing: refused for a COG only; a plain file takes it (and the valid puts behind it overwrite)
    for rel in ([128, 128], [256, 0]):
        got = _outcome(tmp_path, cog, "extent", "", two, dict(rel=rel, extent_bytes=256 + max(n0, n1)))
        assert got == ((-1, True, "ok") if cog else (0, True, "ok")), rel


@pytest.mark.parametrize("kind", ["tile", "tiles", "extent"])
def test_cog_order_refusals_leave_the_writer_usable(tmp_path, kind):
    """A tile index not above the last one, and a level coarser than the current one: refused by all three puts, the
    file stays intact and complete once the remaining tiles went in."""
    again = [(1, 0, _blob(0, 1, 0))]
    assert _outcome(tmp_path, True, kind, "", again, {}, before=2) == (-1, True, "ok")
    below = [(0, 0, _blob(0, 0, 0))]
    assert _outcome(tmp_path, True, kind, "", below, {}, before=2) == (-1, True, "ok")
    coarser = [(0, 0, _blob(1, 0, 0))]
    assert _outcome(tmp_path, True, kind, "", coarser, {}, before=1, level=1) == (-1, True, "ok")
    assert _outcome(tmp_path, True, kind, "", coarser, {}, before=0, level=2) == (-1, True, "ok")
    if kind != "tile":                                          # descending inside one call
        desc = [(2, 0, _blob(0, 2, 0)), (1, 0, _blob(0, 1, 0))]
        assert _outcome(tmp_path, True, kind, "", desc, {}) == (-1, True, "ok")


# ---- 3. what opening a hand-made file says ----------------------------------------------------------------------

def _classic(ents, n_entries=None, magic=42, mark=b"II", pixels=bytes(range(1, 13))):
    """A little-endian classic TIFF: 8 header bytes, the pixels, one directory of (tag, type, values) entries."""
    fmt = {3: "H", 4: "I"}
    ifd_pos = 8 + len(pixels) + (len(pixels) & 1)
    n = len(ents) if n_entries is None else n_entries
    ifd, extra = bytearray(struct.pack("<H", n)), bytearray()
    extra_pos = ifd_pos + 2 + len(ents) * 12 + 4
    for tag, typ, vals in sorted(ents):
        payload = struct.pack("<" + fmt[typ] * len(vals), *vals)
        ifd += struct.pack("<HHI", tag, typ, len(vals))
        if len(payload) <= 4:
            ifd += payload.ljust(4, b"\0")
        else:
            ifd += struct.pack("<I", extra_pos + len(extra))
            extra += payload
    ifd += struct.pack("<I", 0)
    return mark + struct.pack("<HI", magic, ifd_pos) + pixels + (b"\0" if len(pixels) & 1 else b"") + bytes(ifd + extra)


def _strip_ents(**change):
    """A 4 x 3 raster in one uncompressed strip at offset 8."""
    e = {256: (4, [4]), 257: (4, [3]), 258: (3, [8]), 259: (3, [1]), 262: (3, [1]), 273: (4, [8]), 277: (3, [1]),
         278: (4, [3]), 279: (4, [12])}
    for tag, v in change.items():
        if v is None:
            del e[int(tag[1:])]
        else:
            e[int(tag[1:])] = v
    return [(tag, typ, vals) for tag, (typ, vals) in e.items()]


STRUCTURE = "gdal open failed: <path> (unreadable or unsupported TIFF structure)"
E_STRUCTURE, E_MISSING, E_NOT_BYTE, E_NO_IFD = 1, 2, 3, 4
TILED_NO_WIDTH = _strip_ents(t273=None, t278=None, t279=None, t323=(3, [16]), t324=(4, [8]), t325=(4, [12]))
TWO_STRIPS_ONE_LISTED = _strip_ents(t278=(4, [2]))
OPEN_CASES = {
    "missing": (None, 0, E_MISSING, "gdal open failed: <path>"),
    "7 bytes": (b"II*\0\x08\0\0", 0, E_STRUCTURE, "gdal open failed: <path>"),
    "bad byte-order mark": (_classic(_strip_ents(), mark=b"IM"), 0, E_STRUCTURE, "gdal open failed: <path> (not a TIFF)"),
    "magic 44": (_classic(_strip_ents(), magic=44), 0, E_STRUCTURE, STRUCTURE),
    "0 entries": (_classic(_strip_ents(), n_entries=0), 0, E_STRUCTURE, STRUCTURE),
    "4097 entries": (_classic(_strip_ents(), n_entries=4097), 0, E_STRUCTURE, STRUCTURE),
    "level 1 of one directory": (_classic(_strip_ents()), 1, E_NO_IFD, "gdal open failed: <path> has no directory 1"),
    "16 bits per sample": (_classic(_strip_ents(t258=(3, [16]))), 0, E_NOT_BYTE,
                           "gdal open failed: <path> (16 bits per sample; only Byte rasters are supported)"),
    "compression 7": (_classic(_strip_ents(t259=(3, [7]))), 0, E_STRUCTURE,
                      "gdal open failed: <path> (TIFF compression 7 not supported)"),
    "tiled without a tile width": (_classic(TILED_NO_WIDTH), 0, E_STRUCTURE, STRUCTURE),
    "fewer chunks than across x down": (_classic(TWO_STRIPS_ONE_LISTED), 0, E_STRUCTURE, STRUCTURE),
}


@pytest.mark.parametrize("case", list(OPEN_CASES))
def test_open_reader_outcome_of_a_hand_made_file(tmp_path, case):
    data, level, why, message = OPEN_CASES[case]
    p = str(tmp_path / "f.tif")
    if data is not None:
        open(p, "wb").write(data)
    t = Tiff(p, level)
    assert not t.h and t.why.value == why and t.message() == message.replace("<path>", p)


def test_open_reader_takes_the_plain_hand_made_file(tmp_path):
    """The file the refusals above are variations of opens and reads."""
    p = str(tmp_path / "f.tif")
    open(p, "wb").write(_classic(_strip_ents()))
    t = Tiff(p)
    assert t.h and t.why.value == E_STRUCTURE and t.info() == (4, 3, [0, 1, 0, 0, 0, 1])
    assert t.read(0, 0, 4, 3)[1].reshape(-1).tolist() == list(range(1, 13))
    t.close()


@pytest.mark.parametrize("kw", [dict(bigtiff=True), dict(big_endian=True), dict(bigtiff=True, big_endian=True)], ids=str)
@pytest.mark.parametrize("shape", ["tiles4x3", "strips3"])
def test_open_reader_takes_bigtiff_and_big_endian_files(tmp_path, shape, kw):
    p = str(tmp_path / "f.tif")
    tiffutil.write_tiff(p, IMG, gt=GT, compression=8, **SHAPES[shape], **kw)
    t = Tiff(p)
    assert t.h and t.why.value == E_STRUCTURE and t.message() == "" and t.info() == (W, H, GT)
    assert np.array_equal(t.read(0, 0, W, H)[1], IMG)
    t.close()
    t = Tiff(p, 1)
    assert not t.h and t.why.value == E_NO_IFD and t.message() == "gdal open failed: %s has no directory 1" % p
