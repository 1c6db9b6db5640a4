"""The tiles and the readers of tests/test_gpu_soil_readers.py, and their numpy references (checked on the CPU by
tests/test_soil_reader_references.py).

A TILE is a landcover strip, a soil window and the two index maps (tests/test_gpu_soil_tables.Tile); tile_specs()
names the ones of cases A to G.  A READER is one of the eight paths that read the code bytes of the prepared tile
(strip, verify, histogram, zonal, overview, fused, aggregate and grid, all held to the cases A to I):
it allocates and uploads everything it needs when it is made, launch(stream) queues its work, and check() compares
what came back with numpy and the oracle -- never with another GPU path.
"""
import math
import zlib

import numpy as np

from gcn10_amd import gpu, host
from tests import aggutil, gridutil, stormutil
from tests.fullblock import average_levels
from tests.test_gpu_grid import maps
from tests.test_gpu_soil_tables import K1, Tile, _with_complex_group, clamp_columns
from tests.test_gpu_stats import model_histogram, soil_code
from tests.util import ESA_NASTY, HSG_NASTY

GUARD = 256
HIST = 16 * 256
NONE = gpu.VERIFY_NONE
READERS = ("strip", "verify", "histogram", "zonal", "overview", "fused", "aggregate", "grid")
SHIFTED = (3, 1, 4, 0)      # case G: byte offsets of esa, coarse, ci and cj in their buffers (ci: not 16-byte aligned)
SHIFTED_MAPS = (0, 1, 4, 0)     # the same with the landcover aligned, so that strips may read the compact words
_REFERENCES = {}            # spec id -> (rasters, soils) of the oracle, computed once and shared
OUTSIDE = (-1, -5, 64, 64 + 7, 2 ** 31 - 1, -2 ** 31, 1 << 24, -(1 << 24))       # case E of the soil-table tests, hsx = 64


# ---- the tiles -------------------------------------------------------------------------------------------------

def _default_map(W, hsx):
    return (np.arange(W) * hsx // W).astype(np.int32)


def outside_map(kind, W=2048, hsx=64):
    """The "runs" and "scattered" maps of case E of tests/test_gpu_soil_tables.py: columns outside the window."""
    ci = _default_map(W, hsx)
    outside = np.array(OUTSIDE, np.int32)
    if kind == "runs":
        ci[:32] = np.repeat(outside[:2], 16)
        ci[-48:] = np.repeat(outside[2:5], 16)
    else:
        at = np.random.default_rng(3).choice(W, size=200, replace=False)
        ci[at] = outside[np.arange(200) % outside.size]
        ci[0], ci[W - 1] = -1, hsx
    return ci


def tile_specs():
    """{id: dict(seed, W, H, hsx, hsy, ci)} of the tiles A to G, in the order of the cases (ci None: Tile's own
    monotone map).  G's tiles are uploaded at byte offsets (SHIFTED); H and I are sequences, made by their tests."""
    W = 2048
    s = {}
    s["A-decreasing"] = dict(W=W, H=40, hsx=90, hsy=6, ci=(90 - 1 - np.arange(W) * 90 // W).astype(np.int32))
    s["A-zig-zag"] = dict(W=W, H=40, hsx=90, hsy=6,
                          ci=((np.arange(W) // 5) % 2 * 40 + np.arange(W) * 40 // W).astype(np.int32))
    s["A-constant"] = dict(W=W, H=40, hsx=90, hsy=6, ci=np.full(W, 17, np.int32))
    s["B-runs"] = dict(W=W, H=40, hsx=64, hsy=6, ci=outside_map("runs"))
    s["B-scattered"] = dict(W=W, H=40, hsx=64, hsy=6, ci=outside_map("scattered"))
    s["C-first"] = dict(W=W, H=40, hsx=64, hsy=5, ci=_with_complex_group(W, 64, 0))
    s["C-last"] = dict(W=W, H=40, hsx=64, hsy=5, ci=_with_complex_group(W, 64, 127))
    s["C-holds-column-W-1"] = dict(W=2051, H=40, hsx=64, hsy=5, ci=_with_complex_group(2051, 64, 128))
    for hsx, hsy in ((1, 1), (1, 4), (70, 1)):
        s["D-%dx%d" % (hsx, hsy)] = dict(W=W, H=40, hsx=hsx, hsy=hsy, ci=None)
    s["D-narrow-cells"] = dict(W=W, H=40, hsx=3000, hsy=6, ci=None)
    for w in (5, 16, 17, 31):
        s["E-%d" % w] = dict(W=w, H=3, hsx=3, hsy=2, ci=None)
    for w in (2047, 2049):
        s["E-%d" % w] = dict(W=w, H=40, hsx=90, hsy=6, ci=None)
    s["F-300x270"] = dict(W=300, H=270, hsx=14, hsy=13, ci=None)
    for w in (2048, 2051):
        s["G-%d" % w] = dict(W=w, H=40, hsx=90, hsy=6, ci=None)
    for i, k in enumerate(s):
        s[k]["seed"] = 100 + i
    return s


SPECS = tile_specs()
# case I: three tiles prepared one after the other on one context; the second is smaller, the third as wide as the first
CASE_I = (dict(seed=1, W=2048, H=40, hsx=90, hsy=6), dict(seed=2, W=1040, H=40, hsx=50, hsy=5),
          dict(seed=3, W=2048, H=40, hsx=90, hsy=6))


def case_i_soils():
    """The soil class of every pixel of the three tiles, as Tile draws and resamples it (no device needed)."""
    out = []
    for s in CASE_I:
        rng = np.random.default_rng(s["seed"])
        rng.choice(ESA_NASTY, size=(s["H"], s["W"]))            # Tile draws the landcover first
        coarse = rng.choice(HSG_NASTY, size=(s["hsy"], s["hsx"])).astype(np.uint8)
        cj = np.minimum((np.arange(s["H"]) + 3) * s["hsy"] // (s["H"] + 3), s["hsy"] - 1)
        out.append(coarse[cj][:, _default_map(s["W"], s["hsx"])])
    return out


class _Shifted:
    """A device array that begins `offset` bytes into its allocation."""

    def __init__(self, eng, arr, offset):
        a = np.ascontiguousarray(arr)
        self.base, self.nbytes = eng.alloc(a.nbytes + offset), a.nbytes
        self.ptr = self.base.ptr + offset
        eng.h2d(self.ptr, a)
        eng.sync()

    def at(self, offset):
        assert 0 <= offset <= self.nbytes
        return self.ptr + offset

    def close(self):
        self.base.close()


class ReaderTile(Tile):
    """A Tile whose oracle rasters are shared by every test that builds the same one (key), optionally uploaded at
    byte offsets (esa, coarse, ci, cj) inside fresh allocations."""

    def __init__(self, eng, tables, seed, W, H, hsx, hsy, ci=None, cj=None, key=None, offsets=None):
        self.offsets = offsets
        super().__init__(eng, tables, seed, W, H, hsx, hsy, ci=ci, cj=cj)
        if key is not None:
            self._want, self._soil = _REFERENCES.setdefault(key, ({}, {}))

    def upload_inputs(self):
        if self.offsets is None:
            return super().upload_inputs()
        return [_Shifted(self.eng, a, o) for a, o in zip((self.esa, self.coarse, self.ci, self.cj), self.offsets)]


def make_tile(eng, tables, name, offsets=None):
    return ReaderTile(eng, tables, key=name, offsets=offsets, **SPECS[name])


class _NoDevice:
    """In place of the engine where only the host side of a tile is wanted: nothing is uploaded."""

    def upload(self, a):
        return None


def host_tile(tables, name):
    """The tile `name` without a device: its inputs and the oracle's rasters, for the CPU checks of the references."""
    return ReaderTile(_NoDevice(), tables, key=name, **SPECS[name])


# ---- references ------------------------------------------------------------------------------------------------

def pair_keys(esa, soil):
    """bin * 256 + landcover of every pixel: the index of its counter in a pair histogram."""
    codes = gpu.pair_histogram_codes()
    lut = np.zeros(256, np.int64)
    for b in range(9):
        lut[codes[b]] = b
    return lut[soil_code(soil)] * 256 + esa.astype(np.int64)


def zone_counts(esa, soil, spans, n_zones):
    """uint64[n_zones][16 * 256]: the pair counts of the pixels every zone's spans name, by numpy."""
    key = pair_keys(esa, soil)
    want = np.zeros((n_zones, HIST), np.uint64)
    for s in spans:
        np.add.at(want[s["zone"]], key[s["y"], s["x0"]:s["x1"]], 1)
    return want


def reader_spans(W, H):
    """Two zones with ragged edges, one span per row each: zone 0 on the left (row 0 starts at column 0, the last
    row is a span that starts and ends inside the first 16-px group), zone 1 on the right (row 0 ends at W)."""
    sp = []
    for y in range(H):
        a0 = 0 if y == 0 else (7 * y) % min(23, max(1, W // 4))
        b0 = min(W, max(a0 + 1, W // 2 - (5 * y) % 11))
        if y == H - 1 and W >= 3:
            a0, b0 = 1, min(W - 1, 3)
        sp.append((y, a0, b0, 0))
        a1 = min(W - 1, max(b0, W // 2 + 1 + (3 * y) % 9))
        b1 = W if y == 0 else min(W, max(a1 + 1, W - (11 * y) % 17))
        sp.append((y, a1, b1, 1))
    a = np.array(sp, host.ZONE_SPAN_DTYPE)
    return a[np.lexsort((a["x0"], a["y"], a["zone"]))]


def strips_inside_a_soil_row(cj):
    """[(y0, rows)]: the tile in two strips, the second starting inside a soil row (one strip for a single row)."""
    H = len(cj)
    inside = [y for y in range(1, H) if cj[y] == cj[y - 1]]
    assert inside or H == 1, "no row of this tile lies inside a soil row"
    if not inside:
        return [(0, H)]
    y = min(inside, key=lambda v: abs(v - H // 2))
    return [(0, y), (y, H - y)]


def selected(cond_mask, table_mask):
    return [c * 9 + k for c in range(2) for k in range(9) if cond_mask >> c & 1 and table_mask >> k & 1]


AGG_SMALL, AGG_WIDE = "aggregate_small_kernel", "aggregate_kernel"      # the kernels for f < 16 and f >= 16


def aggregate_passes(W, cj):
    """The passes of AggregateReader over a tile W wide whose rows have the soil rows cj: dicts of the factor f, the
    columns [x0, x1), the masks, the strips [(y0, rows)] of one call each, and the kernel that runs them.

      f = 3   all columns, all rasters, the two strips of strips_inside_a_soil_row: the kernel for f < 16
      f = 16  all columns, all rasters, ONE ROW per call: a cell is 16 pixels of one row, so that every soil byte is
              1/16 of a cell (an area mean over a whole tile hides a wrong byte; tests/test_soil_reader_references.py
              counts what each pass lets through)
      f = 25  a subset of the rasters in the two strips: the row walk across changing soil rows, with a first and
              a last column inside a 16-pixel group: [1, W - 1), or [1, W - 2) where W - 1 is a multiple of 16

    A strip's cells are reduced by themselves, whatever the factor: that a strip starts at a cell-row boundary is the
    caller's convention, nothing gcn10_gpu_aggregate knows."""
    two, by_row = strips_inside_a_soil_row(cj), [(y, 1) for y in range(len(cj))]
    x0, x1 = (1, W - 1) if W >= 3 else (0, W)
    if x1 % 16 == 0 and x1 - 1 > x0:
        x1 -= 1
    passes = [dict(f=3, x0=0, x1=W, masks=(3, 0x1FF), strips=two),
              dict(f=16, x0=0, x1=W, masks=(3, 0x1FF), strips=by_row),
              dict(f=25, x0=x0, x1=x1, masks=(2, 0x0A1), strips=two)]
    for p in passes:
        p["form"] = AGG_SMALL if p["f"] < 16 else AGG_WIDE
        p["sel"] = selected(*p["masks"])
        p["Wa"] = aggutil.cells(p["x1"] - p["x0"], p["f"])
        p["cell_rows"] = [aggutil.cells(rows, p["f"]) for _y0, rows in p["strips"]]
    return passes


def reduce_strips(raster, x0, x1, f, strips):
    """uint8[sum of the strips' cell rows][cells]: every strip reduced by itself (aggutil.reduce_raster), the cell
    rows of a strip behind those of the strip before."""
    return np.vstack([aggutil.reduce_raster(raster[y0:y0 + rows], x0, x1, f) for y0, rows in strips])


# the two weight tables of every GridReader: the low and the high byte of "random" both depend on the value (with
# "all 65535" only whether a value is 255 would show), and "50 mm" is a real storm's
GRID_TABLES = np.stack([stormutil.POOL["random"], stormutil.POOL["50 mm"]])
GRID_LEAD, GRID_TRAIL = (5, 3), (3, 2)      # columns and rows of -1 before and behind the cells of the `storms` pass


def grid_edges(W, H):
    """(lead, trail) of the `storms` pass: -1 columns only where W >= 32, -1 rows only where H >= 8."""
    wide, tall = W >= 32, H >= 8
    return ((GRID_LEAD[0] * wide, GRID_LEAD[1] * tall), (GRID_TRAIL[0] * wide, GRID_TRAIL[1] * tall))


def grid_passes(W, H, cj):
    """The passes of GridReader over a W x H tile whose rows have the soil rows cj: dicts of the maps cellx and celly,
    the cells ncx x ncy, the masks, the entry point `call`, the weight tables `ws` of its words beyond {s, n} and the
    strips [(y0, rows)] of one call each, all adding into the same words.

      rows    cells of 8 px of ONE row (the narrowest the kernel's three-masks rule allows), all rasters, pairs, one
              call over the whole tile: every soil byte is at least 1/8 of a cell's sum
      storms  cells of 25 x 25.6 px, -1 columns and rows around them (grid_edges), a subset of the rasters, 2 + 2 words
              with GRID_TABLES, in the two strips of strips_inside_a_soil_row: the row walk across changing soil rows,
              a strip that starts inside a soil row and inside a cell row, -1 runs that end inside a 16-px group"""
    lead, trail = grid_edges(W, H)
    sx, sy = maps(W, H, 25, 25.6, lead, trail)
    passes = [dict(name="rows", cellx=(np.arange(W) // 8).astype(np.int32), celly=np.arange(H, dtype=np.int32),
                   masks=(3, 0x1FF), call="grid_sums", ws=GRID_TABLES[:0], strips=[(0, H)]),
              dict(name="storms", cellx=sx, celly=sy, masks=(2, 0x0A1), call="grid_sums_storms", ws=GRID_TABLES,
                   strips=strips_inside_a_soil_row(cj))]
    for p in passes:
        p["sel"] = selected(*p["masks"])
        p["ncx"], p["ncy"], p["words"] = int(p["cellx"].max()) + 1, int(p["celly"].max()) + 1, 2 + len(p["ws"])
    return passes


def weighted_rows_pass(W, H, cj):
    """The `rows` pass as triples of one table, "random", for gcn10_gpu_grid_sums_weighted."""
    p = grid_passes(W, H, cj)[0]
    p.update(name="rows, weighted", call="grid_sums_weighted", ws=GRID_TABLES[:1], words=3)
    return p


def grid_words(p, rasters):
    """int64[n_sel][ncy][ncx][words]: what the pass's calls add up to over rasters[r], strip by strip."""
    acc = np.zeros((len(p["sel"]), p["ncy"], p["ncx"], p["words"]), np.int64)
    for q, r in enumerate(p["sel"]):
        for y0, rows in p["strips"]:
            part, celly = rasters[r][y0:y0 + rows], p["celly"][y0:y0 + rows]
            if len(p["ws"]):
                stormutil.add_words(acc[q], part, p["cellx"], celly, p["ws"])
            else:
                gridutil.add_sums(acc[q], part, p["cellx"], celly)
    return acc


# ---- the readers -----------------------------------------------------------------------------------------------

class Reader:
    def __init__(self, tile):
        self.t, self.eng, self.bufs = tile, tile.eng, []
        self.esa, self.cj = tile.bufs[0], tile.bufs[3]

    def alloc(self, n):
        self.bufs.append(self.eng.alloc(n))
        return self.bufs[-1]

    def upload(self, a):
        self.bufs.append(self.eng.upload(a))
        return self.bufs[-1]

    def close(self):
        for b in self.bufs:
            b.close()
        self.bufs = []


class StripReader(Reader):
    """cn_strip with compact_soil = 0 (all 18 rasters from the code bytes), then one raster at an odd address, which
    takes the byte kernel.  The option is switched after prepare_tile, so the bytes are not made by it."""
    name = "strip"

    def __init__(self, tile):
        super().__init__(tile)
        self.n = tile.W * tile.H
        self.slot = (self.n + 1 + GUARD + 255) & ~255
        self.out = self.alloc(19 * self.slot)

    def launch(self, stream=None):
        e, t = self.eng, self.t
        e.memset(self.out.ptr, 0xA5, 19 * self.slot, stream)
        e.set_option("compact_soil", 0)
        try:
            e.cn_strip(self.esa.ptr, t.W, t.H, self.cj.ptr, 3, 0x1FF, [self.out.at(r * self.slot) for r in range(18)],
                       stream)
            ptrs = [None] * 18
            ptrs[K1] = self.out.at(18 * self.slot + 1)
            e.cn_strip(self.esa.ptr, t.W, t.H, self.cj.ptr, 1, 1 << K1, ptrs, stream)
            self.kernel = e.last_kernel_name()
        finally:
            e.set_option("compact_soil", 1)

    def check(self):
        t, n = self.t, self.n
        img = self.eng.download(self.out.ptr, (19, self.slot))
        assert self.kernel == "cn_strip_bytes"
        for r in range(18):
            np.testing.assert_array_equal(img[r, :n].reshape(t.H, t.W), t.want(r), err_msg="strip: raster %d" % r)
            assert (img[r, n:] == 0xA5).all(), "strip: raster %d wrote behind its last pixel" % r
        np.testing.assert_array_equal(img[18, 1:1 + n].reshape(t.H, t.W), t.want(K1), err_msg="byte kernel")
        assert img[18, 0] == 0xA5 and (img[18, 1 + n:] == 0xA5).all(), "the byte kernel wrote outside its raster"


class VerifyReader(Reader):
    """verify_strip in two strips, over the oracle's rasters and over the same with pixel (H-1, W-1) changed."""
    name = "verify"

    def __init__(self, tile):
        super().__init__(tile)
        t = tile
        self.stride = t.W + 5
        self.want = np.stack([t.want(r) for r in range(18)])
        clean = np.random.default_rng(t.W).integers(0, 256, size=(18, t.H, self.stride), dtype=np.uint8)
        clean[:, :, :t.W] = self.want
        self.planted = clean.copy()
        self.planted[:, t.H - 1, t.W - 1] ^= 0x80
        self.dev = [self.upload(clean), self.upload(self.planted)]
        self.counts = [self.eng.verify_counts_alloc(), self.eng.verify_counts_alloc()]
        self.bufs += self.counts
        self.strips = strips_inside_a_soil_row(t.cj)

    def launch(self, stream=None):
        t = self.t
        for dev, counts in zip(self.dev, self.counts):
            for y0, rows in self.strips:
                ptrs = [dev.ptr + (r * t.H + y0) * self.stride for r in range(18)]
                self.eng.verify_strip(self.esa.at(y0 * t.W), t.W, rows, self.cj.at(4 * y0), 3, 0x1FF, ptrs,
                                      self.stride, y0, counts.ptr, stream)

    def check(self):
        t = self.t
        clean = self.eng.verify_counts(self.counts[0].ptr)
        assert clean["mismatches"].tolist() == [0] * 18, "verify: the oracle's rasters do not verify clean"
        assert clean["first"].tolist() == [NONE] * 18
        y, x = t.H - 1, t.W - 1
        planted = self.eng.verify_counts(self.counts[1].ptr)
        for r in range(18):
            assert planted[r].tolist() == (1, (y << 32) | x, int(self.want[r, y, x]), int(self.planted[r, y, x])), r


class HistogramReader(Reader):
    name = "histogram"

    def __init__(self, tile):
        super().__init__(tile)
        self.hist = self.alloc(HIST * 8)

    def launch(self, stream=None):
        t = self.t
        self.eng.memset(self.hist.ptr, 0, HIST * 8, stream)
        self.eng.pair_histogram(self.esa.ptr, t.W, t.H, self.cj.ptr, self.hist.ptr, stream)

    def check(self):
        got = self.eng.download(self.hist.ptr, (HIST,), np.uint64)
        np.testing.assert_array_equal(got, model_histogram(self.t.esa, self.t.soil), err_msg="pair histogram")


class ZonalReader(Reader):
    """zonal_pair_histogram_device over reader_spans, cut into items by the host builder."""
    name = "zonal"

    def __init__(self, tile):
        super().__init__(tile)
        t = tile
        self.spans = reader_spans(t.W, t.H)
        s2, items = host.zone_items(self.spans)
        assert ((s2["y"] >= 0) & (s2["y"] < t.H) & (s2["x0"] >= 0) & (s2["x0"] < s2["x1"]) & (s2["x1"] <= t.W) &
                (s2["zone"] >= 0) & (s2["zone"] < 2)).all()
        assert int(items["n_spans"].sum()) == s2.size
        self.n_items = items.size
        self.dev = [self.upload(s2), self.upload(items)]
        self.hist = self.alloc(2 * HIST * 8)

    def launch(self, stream=None):
        t = self.t
        self.eng.memset(self.hist.ptr, 0, 2 * HIST * 8, stream)
        self.eng.zonal_pair_histogram_device(self.esa.ptr, t.W, t.H, self.cj.ptr, self.dev[0].ptr, self.dev[1].ptr,
                                             self.n_items, 2, self.hist.ptr, stream)

    def check(self):
        got = self.eng.download(self.hist.ptr, (2, HIST), np.uint64)
        np.testing.assert_array_equal(got, zone_counts(self.t.esa, self.t.soil, self.spans, 2), err_msg="zonal")


class OverviewReader(Reader):
    """overview_average of all 18 rasters in strips of 256 rows, guard bytes around every level."""
    name = "overview"

    def __init__(self, tile):
        super().__init__(tile)
        t = tile
        self.L = max(host.cog_levels(t.W, t.H), 1)
        self.sizes = [(math.ceil(t.H / 2 ** k), math.ceil(t.W / 2 ** k)) for k in range(1, self.L + 1)]
        self.offs, self.total = [], GUARD
        for _q in range(18):
            for h, w in self.sizes:
                self.offs.append(self.total)
                self.total += h * w + GUARD
        self.out = self.alloc(self.total)

    def launch(self, stream=None):
        t = self.t
        self.eng.memset(self.out.ptr, 0xA5, self.total, stream)
        ptrs = [self.out.ptr + o for o in self.offs]
        for y0 in range(0, t.H, 256):
            self.eng.overview_average(self.esa.ptr, t.W, t.H, y0, min(256, t.H - y0), self.cj.ptr, 3, 0x1FF, self.L,
                                      ptrs, stream)

    def check(self):
        got = self.eng.download(self.out.ptr, (self.total,))
        guard = np.ones(self.total, bool)
        for r in range(18):
            model = average_levels(self.t.want(r), self.L)
            for k, (h, w) in enumerate(self.sizes):
                o = self.offs[r * self.L + k]
                guard[o:o + h * w] = False
                np.testing.assert_array_equal(got[o:o + h * w].reshape(h, w), model[k],
                                              err_msg="overview: raster %d level %d" % (r, k + 1))
        assert (got[guard] == 0xA5).all(), "overview: a byte outside the level rasters was written"


class FusedReader(Reader):
    """deflate_fused, all 18 rasters and a subset.  The face downloads the streams: launch() returns when they are
    there, so this reader synchronises its stream (and the device, when it frees its arena)."""
    name = "fused"
    MASKS = ((3, 0x1FF), (2, 0x0A1))

    def launch(self, stream=None):
        t = self.t
        self.res = [self.eng.deflate_fused(self.esa.ptr, t.W, t.H, self.cj.ptr, cm, tm, stream) for cm, tm in self.MASKS]

    def check(self):
        t = self.t
        across, down = (t.W + 255) // 256, (t.H + 255) // 256
        for (cm, tm), (data, table, used) in zip(self.MASKS, self.res):
            sel = selected(cm, tm)
            assert table.shape == (len(sel), down, across, 2)
            for j, r in enumerate(sel):
                want = np.zeros((down * 256, across * 256), np.uint8)
                want[:t.H, :t.W] = t.want(r)
                for ty in range(down):
                    for tx in range(across):
                        off, size = int(table[j, ty, tx, 0]), int(table[j, ty, tx, 1])
                        assert off != 0xFFFFFFFF and 0 < size and off + size <= used, (cm, tm, r, ty, tx)
                        exp = want[ty * 256:(ty + 1) * 256, tx * 256:(tx + 1) * 256]
                        assert zlib.decompress(data[off:off + size].tobytes()) == exp.tobytes(), \
                            "fused %#x/%#x: raster %d tile (%d, %d)" % (cm, tm, r, ty, tx)


class AggregateReader(Reader):
    """gcn10_gpu_aggregate in the passes of aggregate_passes -- both kernels, every column in cells small enough to
    show it -- into poisoned rasters: spare bytes behind every row of cells and a guard around every raster."""
    name = "aggregate"
    SPARE = 7

    def __init__(self, tile):
        super().__init__(tile)
        self.passes = aggregate_passes(tile.W, tile.cj)
        self.total = GUARD
        for p in self.passes:
            p["stride"], p["offs"] = p["Wa"] + self.SPARE, []
            for _r in p["sel"]:
                p["offs"].append(self.total)
                self.total += sum(p["cell_rows"]) * p["stride"] + GUARD
        self.out = self.alloc(self.total)

    def launch(self, stream=None):
        t = self.t
        self.eng.memset(self.out.ptr, 0xA5, self.total, stream)
        for p in self.passes:
            cy = 0
            for (y0, rows), n in zip(p["strips"], p["cell_rows"]):
                ptrs = [self.out.at(o + cy * p["stride"]) for o in p["offs"]]
                self.eng.aggregate(self.esa.at(y0 * t.W), t.W, rows, self.cj.at(4 * y0), p["x0"], p["x1"], p["f"],
                                   p["masks"][0], p["masks"][1], ptrs, p["stride"], stream)
                cy += n

    def check(self):
        t = self.t
        got = self.eng.download(self.out.ptr, (self.total,))
        poison = np.ones(self.total, bool)
        for p in self.passes:
            Ha, Wa, stride = sum(p["cell_rows"]), p["Wa"], p["stride"]
            for o, r in zip(p["offs"], p["sel"]):
                cells = got[o:o + Ha * stride].reshape(Ha, stride)[:, :Wa]
                poison[o:o + Ha * stride].reshape(Ha, stride)[:, :Wa] = False
                want = reduce_strips(t.want(r), p["x0"], p["x1"], p["f"], p["strips"])
                bad = np.argwhere(cells != want).tolist()
                at = tuple(bad[0]) if bad else None
                assert not bad, "aggregate f=%d columns [%d, %d) in %d strips, raster %d: %d cells differ, first " \
                    "(cell row, cell) = %s: got %d, want %d" % (p["f"], p["x0"], p["x1"], len(p["strips"]), r, len(bad),
                                                                at, cells[at], want[at])
        assert (got[poison] == 0xA5).all(), "aggregate: a byte outside the cells was written"


class GridReader(Reader):
    """gcn10_gpu_grid_sums and gcn10_gpu_grid_sums_storms in the passes of grid_passes, into words that are zero
    inside a poisoned buffer (the kernels ADD): a guard around every pass's words.  Every GridReader sets the same
    weight tables when it is made -- set_weight_tables is synchronous, and a set_tables before has voided them -- so
    launch() only queues work and two of them do not disturb each other."""
    name = "grid"

    def __init__(self, tile):
        super().__init__(tile)
        self.passes = self.set_weights_and_passes()
        self.total = GUARD
        for p in self.passes:
            p["off"], p["nbytes"] = self.total, len(p["sel"]) * p["ncy"] * p["ncx"] * p["words"] * 8
            p["dev"] = (self.upload(p["cellx"]), self.upload(p["celly"]))
            self.total += p["nbytes"] + GUARD
        self.out = self.alloc(self.total)

    def set_weights_and_passes(self):
        t = self.t
        self.eng.set_weight_tables(GRID_TABLES)
        return grid_passes(t.W, t.H, t.cj)

    def launch(self, stream=None):
        t = self.t
        self.eng.memset(self.out.ptr, 0xA5, self.total, stream)
        for p in self.passes:
            self.eng.memset(self.out.at(p["off"]), 0, p["nbytes"], stream)
            for y0, rows in p["strips"]:
                getattr(self.eng, p["call"])(self.esa.at(y0 * t.W), t.W, rows, self.cj.at(4 * y0), p["dev"][0].ptr,
                                             p["dev"][1].at(4 * y0), p["ncx"], p["ncy"], p["masks"][0], p["masks"][1],
                                             self.out.at(p["off"]), stream)

    def check(self):
        t = self.t
        got = self.eng.download(self.out.ptr, (self.total,))
        poison = np.ones(self.total, bool)
        for p in self.passes:
            poison[p["off"]:p["off"] + p["nbytes"]] = False
            words = got[p["off"]:p["off"] + p["nbytes"]].view(np.uint64).astype(np.int64)
            want = grid_words(p, {r: t.want(r) for r in p["sel"]})
            words = words.reshape(want.shape)
            bad = np.argwhere(words != want).tolist()
            at = tuple(bad[0]) if bad else None
            assert not bad, "grid pass '%s' (%s) in %d strips: %d of %d words differ, first in raster %d at (cell row, " \
                "cell, word) = %s: got %d, want %d" % (p["name"], p["call"], len(p["strips"]), len(bad), want.size,
                                                      p["sel"][at[0]], at[1:], words[at], want[at])
        assert (got[poison] == 0xA5).all(), "grid: a byte outside the words was written"


class WeightedGridReader(GridReader):
    """gcn10_gpu_grid_sums_weighted, the kernel of three words, over the `rows` pass with one table.  A context holds
    either one table (set_weights) or the k of set_weight_tables, so this reader is not one of READERS: it cannot run
    beside a GridReader."""
    name = "grid, weighted"

    def set_weights_and_passes(self):
        t = self.t
        self.eng.set_weights(GRID_TABLES[0])
        return [weighted_rows_pass(t.W, t.H, t.cj)]


READER_CLASSES = {c.name: c for c in (StripReader, VerifyReader, HistogramReader, ZonalReader, OverviewReader,
                                      FusedReader, AggregateReader, GridReader)}
assert tuple(READER_CLASSES) == READERS


def run_reader(tile, name, stream=None):
    """The named reader (or a Reader class outside READERS) over the tile: made, launched, awaited, checked, freed."""
    rd = (READER_CLASSES[name] if isinstance(name, str) else name)(tile)
    try:
        rd.launch(stream)
        tile.eng.sync(stream)
        rd.check()
    finally:
        tile.eng.sync(stream)
        rd.close()
