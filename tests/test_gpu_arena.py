"""Every arena byte the three tile encoders write (gcn10_gpu_deflate_strip, gcn10_gpu_lzw_strip,
gcn10_gpu_deflate_fused_strip), against the plain statement of the layout rule in tests/arena_model.py.

The host appends whole extents of the arena to the GeoTIFFs, so the bytes between streams and between rasters are
published: inside [0, ceil_align(cursor)) every byte is part of a stream or zero, and nothing else is touched.  Each
case runs an encoder on an arena poisoned with 0xA5 with a guard behind arena_cap, takes the stream sizes (and, for
the fused encoder, the aliases) from the table, and checks table, cursor and the whole image against the model.
Stream content is decoded once (zlib; the strict TIFF LZW decoder of the suite), not examined further."""
import functools
import os
import zlib

import numpy as np
import pytest

from tests import arena_model as am
from tests import cogcheck
from tests import test_gpu_deflate as tdf
from tests import test_gpu_lzw as tlz

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 4096
#: id -> (encoder, option that selects the form of its placement / bit packing pass, value)
ENCODERS = {"deflate-wave_codes1": ("deflate", "deflate_wave_codes", 1), "deflate-wave_codes0": ("deflate", "deflate_wave_codes", 0),
            "lzw": ("lzw", None, None),
            "fused-emit1": ("fused", "fused_emit", 1), "fused-emit0": ("fused", "fused_emit", 0)}
#: id -> (rows, W, rasters)
SHAPES = {"300x700": (300, 700, 3), "513x1025x18": (513, 1025, 18), "1x1": (1, 1, 2),
          "256x256x1": (256, 256, 1), "256x256x2": (256, 256, 2), "256x256x18": (256, 256, 18),
          "256x15616x18": (256, 15616, 18)}       # 61 tiles each, 1098 streams: K = 2, boundaries on a thread's second entry
KINDS = ("patches", "uniform", "noisy", "patches", "random", "patches", "iid", "noisy")
# for the LZW encoder, whose streams a decoder written in Python reads: the same kinds, fewer of the long streams
KINDS_LZW = tuple({5: "noisy", 11: "random", 17: "iid"}.get(i, ("patches", "uniform", "patches", "patches")[i % 4]) for i in range(32))


def _mixed(H, W, seed, kinds=KINDS):
    """A raster whose tile positions cycle through the generators of the DEFLATE and LZW tests."""
    out = np.zeros((-(-H // 256) * 256, -(-W // 256) * 256), np.uint8)
    k = seed
    for y in range(0, out.shape[0], 256):
        for x in range(0, out.shape[1], 256):
            kind = kinds[k % len(kinds)]
            out[y:y + 256, x:x + 256] = (tlz._rasters("iid", 256, 256, seed * 1000 + k) if kind == "iid"
                                         else tdf._rasters(kind, 256, 256, seed * 1000 + k))
            k += 1
    return np.ascontiguousarray(out[:H, :W])


@functools.lru_cache(maxsize=None)
def _rasters(shape_id, lzw):
    """The distinct rasters of a shape and which of them each of the n pointers names (computed once, never changed)."""
    H, W, n = SHAPES[shape_id]
    if shape_id == "256x15616x18":      # three distinct device buffers cycled through the 18 pointers: a 12 MB upload
        kinds = ("patches", "uniform", "patches", "noisy", "patches", "uniform", "patches", "random", "patches", "uniform", "iid")
        distinct = [_mixed(H, W, 50 + i, KINDS_LZW if lzw else kinds) for i in range(3)]
        return distinct, [(r * 7 + r // 3) % 3 for r in range(n)]
    return [_mixed(H, W, 20 + 3 * r, KINDS_LZW if lzw else KINDS) for r in range(n)], list(range(n))


@functools.lru_cache(maxsize=None)
def _fused_inputs(shape_id):
    """Landcover, soil and index maps of a shape for the fused encoder, and the oracle's rasters.  The left half
    of the soil has no dual class (the undrained rasters alias the drained ones there), a band of the landcover is
    open water (all rasters agree)."""
    from gcn10_amd import host
    from oracle import cn_oracle_c as oc
    from tests.conftest import LOOKUPS
    from oracle import cn_oracle_np as onp
    H, W, n = SHAPES[shape_id]
    rng = np.random.default_rng(H * 7 + W)
    small = rng.choice(np.array([10, 20, 30, 40, 50, 60, 90, 95, 100], np.uint8), size=((H + 7) // 8, (W + 7) // 8))
    esa = np.repeat(np.repeat(small, 8, axis=0), 8, axis=1)[:H, :W].copy()
    noisy = rng.random((H, W)) < 0.2 * (np.arange(W)[None, :] // 256 % 3 == 1)      # every third tile column noisier
    esa[noisy] = rng.choice(np.array([10, 30, 40, 60, 90], np.uint8), size=int(noisy.sum()))
    if W > 1024:
        esa[:, 768:1024] = 80
    hsy, hsx = H // 25 + 2, W // 25 + 2
    coarse = rng.choice(np.array([1, 2, 3, 4], np.uint8), size=(hsy, hsx))
    coarse[:, hsx // 2:] = rng.choice(np.array([0, 1, 2, 11, 12, 13, 14, 255], np.uint8), size=(hsy, hsx - hsx // 2))
    gt = [0.0, 3.0 / W, 0.0, 3.0, 0.0, -3.0 / W]
    sgt = [-0.01, 3.02 / hsx, 0.0, 3.01, 0.0, -3.02 / hsy]
    ci, cj = host.build_index_maps(gt, sgt, W, H, hsx, hsy)
    tables = []
    for hc in onp.HCS:
        for arc in onp.ARCS:
            tables.append(oc.load_lookup_table(os.path.join(LOOKUPS, "default_lookup_%s_%s.csv" % (hc, arc)))[0])
    tables = np.stack(tables)
    cond_mask, table_mask = {1: (1, 0x010), 2: (3, 0x004), 3: (1, 0x111), 18: (3, 0x1FF)}[n]
    want = oc.process_block_mem(esa, gt, coarse, sgt, tables, cond_mask=cond_mask, table_mask=table_mask)
    sel = [r for r in range(18) if (cond_mask >> (r // 9)) & 1 and (table_mask >> (r % 9)) & 1]
    return np.ascontiguousarray(esa), coarse, ci, cj, tables, cond_mask, table_mask, [want[r] for r in sel]


class Case:
    """One encoder on one shape: run(cap) -> (image, table, used); tile(r, t) -> the 65536 bytes stream (r, t) encodes."""

    def __init__(self, engine, enc_id, shape_id):
        self.engine, self.kind, self.option, self.value = (engine,) + ENCODERS[enc_id]
        self.H, self.W, self.n = SHAPES[shape_id]
        self.across = (self.W + 255) // 256
        self.tiles = self.across * ((self.H + 255) // 256)
        self.bufs = []
        if self.kind == "fused":
            esa, coarse, ci, cj, tables, self.cond_mask, self.table_mask, self.want = _fused_inputs(shape_id)
            engine.set_tables(tables)
            self.bufs = [engine.upload(a) for a in (esa, coarse, ci, cj)]
            engine.prepare_tile(self.bufs[1].ptr, coarse.shape[1], coarse.shape[0], self.bufs[2].ptr, self.W)
        else:
            distinct, which = _rasters(shape_id, self.kind == "lzw")
            self.bufs = [engine.upload(a) for a in distinct]
            self.ptrs = [self.bufs[i].ptr for i in which]
            self.want = [distinct[i] for i in which]

    def run(self, seg_align, cap=None):
        e = self.engine
        try:
            e.set_option("arena_segment_align", seg_align)
            if self.option:
                e.set_option(self.option, self.value)
            kw = dict(arena_cap=cap, poison=POISON, guard=GUARD)
            if self.kind == "fused":
                return e.deflate_fused(self.bufs[0].ptr, self.W, self.H, self.bufs[3].ptr, self.cond_mask, self.table_mask, **kw)
            return (e.deflate_rasters if self.kind == "deflate" else e.lzw_strip)(self.ptrs, self.W, self.H, **kw)
        finally:
            e.set_option("defaults", 0)

    def close(self):
        for b in self.bufs:
            b.close()

    def tile(self, r, t):
        return tdf_tile(self.want[r], t // self.across, t % self.across)

    def aliases(self, table):
        """alias_of[r][t] from a full run's table: an entry equal to an earlier raster's entry of the same tile
        position -- legitimate only where the oracle's rasters are equal there."""
        tab = table.reshape(self.n, self.tiles, 2)
        alias = [[None] * self.tiles for _ in range(self.n)]
        if self.kind != "fused":
            return alias
        for r in range(self.n):
            for t in range(self.tiles):
                for q in range(r):
                    if alias[q][t] is None and tuple(tab[q, t]) == tuple(tab[r, t]):
                        assert self.tile(q, t) == self.tile(r, t), "rasters %d and %d share a stream of tile %d but differ" % (q, r, t)
                        alias[r][t] = q
                        break
        return alias


def tdf_tile(img, ty, tx):
    want = np.zeros((256, 256), np.uint8)
    part = img[ty * 256:(ty + 1) * 256, tx * 256:(tx + 1) * 256]
    want[:part.shape[0], :part.shape[1]] = part
    return want.tobytes()


_decoded = {}        # stream bytes -> the tile they decode to: a stream met again (other alignment, other form) is not decoded again


def _decode(kind, stream):
    key = (kind == "lzw", stream)
    if key not in _decoded:
        _decoded[key] = tlz.strict_lzw_decode(stream, 65536)[0] if kind == "lzw" else zlib.decompress(stream)
    return _decoded[key]


def _full_run(case, seg_align):
    """A run with the encoder's own arena bound: everything fits.  Table, cursor and image obey the model, every
    stream decodes to its tile.  Returns (layout, sizes, aliases, image, table)."""
    image, table, used = case.run(seg_align)
    cap = len(image) - GUARD
    tab = table.reshape(case.n, case.tiles, 2)
    assert (tab[..., 0] != 0xFFFFFFFF).all() and (tab[..., 1] > 0).all()
    alias = case.aliases(table)
    sizes = tab[..., 1].astype(np.int64).tolist()
    lay = am.layout(sizes, alias, seg_align, cap)
    am.check(lay, table, used, image, cap, POISON)
    for r in range(case.n):
        for t in range(case.tiles):
            off, size = int(tab[r, t, 0]), int(tab[r, t, 1])
            assert _decode(case.kind, image[off:off + size].tobytes()) == case.tile(r, t), (r, t)
    return lay, sizes, alias, image, tab


@pytest.mark.parametrize("seg_align", [16, 512, 4096])
@pytest.mark.parametrize("shape_id", list(SHAPES))
@pytest.mark.parametrize("enc_id", list(ENCODERS))
def test_every_arena_byte_is_a_stream_a_zero_or_untouched(engine, enc_id, shape_id, seg_align):
    case = Case(engine, enc_id, shape_id)
    try:
        lay, sizes, alias, image, tab = _full_run(case, seg_align)
    finally:
        case.close()
    own = np.array([sizes[r][t] for r in range(case.n) for t in range(case.tiles) if alias[r][t] is None])
    tails = sorted(set((own % 16).tolist()))
    print("%s %s seg_align %d: %d streams, size %% 16 in %s, cursor %d" % (enc_id, shape_id, seg_align, len(own), tails, lay.cursor))
    if shape_id == "256x15616x18":
        assert len(own) == 1098 or case.kind == "fused"
    if shape_id == "513x1025x18":
        # the case cannot pass vacuously: slot tails of every length the emitters have to zero are present
        if case.kind == "lzw":
            assert any(1 <= v <= 12 for v in tails), tails
        else:
            assert set(range(1, 9)) <= set(tails), tails


CAPS = ["last-slot-less-one", "on-a-slot-end", "inside-a-stream-of-the-second-raster", "inside-a-pad", "no-multiple-of-16", "15"]


def _pick_cap(how, lay, case):
    own = sorted((int(o), int(s)) for o, s in {tuple(e) for e in lay.table.reshape(-1, 2).tolist()})
    second = [(o, s) for o, s in own if o >= lay.starts[1] and lay.ends[1] > lay.starts[1]] or own[1:]
    if how == "last-slot-less-one":
        return lay.cursor - 1
    if how == "on-a-slot-end":
        o, s = second[0]
        return o + am.ceil_to(s, 16)
    if how == "inside-a-stream-of-the-second-raster":
        o, s = second[min(1, len(second) - 1)]
        assert s >= 2
        return o + s // 2
    if how == "inside-a-pad":
        r = next(r for r in range(case.n - 1) if lay.starts[r + 1] - lay.ends[r] >= 48)
        return lay.ends[r] + (lay.starts[r + 1] - lay.ends[r]) // 32 * 16
    if how == "no-multiple-of-16":
        return lay.cursor * 2 // 3 // 16 * 16 + 7
    return 15


@pytest.mark.parametrize("seg_align", [4096, 16])
@pytest.mark.parametrize("enc_id", list(ENCODERS))
def test_an_arena_too_small_keeps_what_fits_and_touches_nothing_else(engine, enc_id, seg_align):
    """Caps from a first run with a full arena (the encoders are deterministic): one byte short of the last slot's end,
    exactly on a slot's end, inside a stream of the second raster, inside the pad between two rasters (seg_align
    4096), no multiple of 16, and 15 bytes, where nothing fits and nothing is written.  Table, cursor and image obey
    the model with a guard of 4096 bytes behind the cap; what fits is the full run's stream, byte for byte."""
    case = Case(engine, enc_id, "300x700")
    try:
        full, sizes, alias, full_image, full_tab = _full_run(case, seg_align)
        for how in CAPS:
            if how == "inside-a-pad" and seg_align == 16:
                continue                    # there is no pad to be inside of
            cap = _pick_cap(how, full, case)
            image, table, used = case.run(seg_align, cap)
            assert len(image) == cap + GUARD
            lay = am.layout(sizes, alias, seg_align, cap)
            fits = lay.table[..., 0] != 0xFFFFFFFF
            if how == "15":
                assert not fits.any() and (image == POISON).all()
            else:
                assert fits.any() and not fits.all(), how
            if how == "on-a-slot-end":
                assert any(b == cap or am.ceil_to(b, 16) == cap for _, b in lay.streams)
            try:
                am.check(lay, table, used, image, cap, POISON)
            except AssertionError as e:
                raise AssertionError("cap %d (%s): %s" % (cap, how, e))
            assert used == full.cursor and np.array_equal(lay.table[fits], full.table[fits])
            for a, b in lay.streams:
                assert np.array_equal(image[a:b], full_image[a:b]), (how, a, b)
    finally:
        case.close()


def test_more_streams_than_the_placement_pass_keeps_in_registers(engine):
    """40 968 streams in one launch (18 pointers at one raster of 256 x 582 656: 2276 tiles each): 41 entries per
    thread of deflate_place_kernel, its re-read path.  Every entry, the cursor and the whole 512 MiB image obey the
    model; raster 0's streams inflate to their tiles and the other 17 extents equal raster 0's byte for byte.
    Wall time on an MI355X as pytest --durations reported it: 0.51 s call (profiles/arena/mutation_check.txt)."""
    rng = np.random.default_rng(2024)
    palette = [tdf._rasters(k, 256, 256, 90 + i) for i, k in
               enumerate(("uniform", "zeros", "patches", "patches", "skewed", "manyvals", "rows", "noisy"))]
    pick = rng.choice(len(palette), size=2276, p=[0.2, 0.1, 0.2, 0.2, 0.1, 0.1, 0.07, 0.03])
    H, W, n = 256, 2276 * 256, 18
    raster = np.ascontiguousarray(np.concatenate([palette[i] for i in pick], axis=1))
    assert raster.shape == (H, W)
    cap = 512 << 20
    buf = engine.upload(raster)
    del raster
    try:
        image, table, used = engine.deflate_rasters([buf.ptr] * n, W, H, arena_cap=cap, poison=POISON, guard=GUARD)
    finally:
        engine.set_option("defaults", 0)
        buf.close()
    tab = table.reshape(n, 2276, 2)
    assert tab.shape[0] * tab.shape[1] == 40968 and (tab[..., 0] != 0xFFFFFFFF).all() and used <= cap
    lay = am.layout(tab[..., 1].astype(np.int64).tolist(), None, 4096, cap)
    assert np.array_equal(tab, lay.table)
    am.check(lay, table, used, image, cap, POISON)
    tiles = [p.tobytes() for p in palette]
    for t in range(2276):
        off, size = int(tab[0, t, 0]), int(tab[0, t, 1])
        assert zlib.decompress(image[off:off + size].tobytes()) == tiles[pick[t]], t
    extent = image[:lay.ends[0]]
    for r in range(1, n):
        assert lay.ends[r] - lay.starts[r] == len(extent)
        assert np.array_equal(image[lay.starts[r]:lay.ends[r]], extent), r


# ---- files, end to end: no stray byte between the tiles of a published GeoTIFF ---------------------

def _stray_bytes(path):
    """Bytes between the first tile's start and the last tile's end of a TIFF that lie in no tile (IFDs and tag
    arrays, which the file itself locates, left out): (how many, how many of them are not zero)."""
    with open(path, "rb") as f:
        data = np.frombuffer(f.read(), np.uint8)
    ifds = cogcheck.read_ifds(data.tobytes())
    covered = np.zeros(len(data), bool)
    lo, hi = len(data), 0
    for pos, end, tags, ranges in ifds:
        covered[pos:end] = True
        for a, b in ranges:
            covered[a:b] = True
        for off, cnt in zip(tags[324], tags[325]):
            assert cnt > 0 and off + cnt <= len(data)
            covered[off:off + cnt] = True
            lo, hi = min(lo, off), max(hi, off + cnt)
    between = ~covered[lo:hi]
    return int(between.sum()), int((data[lo:hi][between] != 0).sum())


@pytest.mark.parametrize("direct_io", [0, 1])
@pytest.mark.parametrize("codec", ["deflate-gpu_deflate1", "deflate-gpu_deflate2", "lzw"])
def test_written_files_carry_no_stray_bytes_between_their_tiles(tmp_path, tables, codec, direct_io):
    """What a user sees of the rule: every byte of a written GeoTIFF between its first and its last tile that
    belongs to no tile is zero, for each encoder the program drives, with and without O_DIRECT extents."""
    cfg = {"deflate-gpu_deflate1": "compress=deflate\ngpu_deflate=1\n", "deflate-gpu_deflate2": "compress=deflate\ngpu_deflate=2\n",
           "lzw": "compress=lzw\n"}[codec] + "direct_io=%d\n" % direct_io
    esa, soil = tlz._world(tmp_path, seed=17, extra_cfg=cfg)
    (tmp_path / "ids.txt").write_text("101 103\n")
    out = tlz._run(tmp_path, "-c", "config.txt", "-l", "ids.txt")
    assert out.returncode == 0, out.stderr[-2000:]
    files = sorted(str(p) for c in tlz.CONDS for p in (tmp_path / ("cn_rasters_%s" % c)).iterdir())
    assert len(files) == 36
    gaps = 0
    for p in files:
        n, nonzero = _stray_bytes(p)
        gaps += n
        assert nonzero == 0, "%s: %d of the %d bytes between its tiles are not zero" % (p, nonzero, n)
    print("%s direct_io=%d: %d bytes between tiles, all zero" % (codec, direct_io, gaps))
    assert gaps > 0         # slot tails at least: the check looked at something
