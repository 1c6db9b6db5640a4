"""GPU: the soil of a prepared tile (gcn10_gpu_prepare_tile keeps codes[hsy][hsx], the column map and one compact
word per 16-px column group and soil row; the code bytes are made on demand from that snapshot).  Needs an MI355X.

Expected values: the oracle's calculate_cn / modify_hysogs_data over coarse[cj][:, ci] taken with plain numpy
indexing, and numpy pair counts -- never another GPU path.
"""
import numpy as np
import pytest

from oracle import cn_oracle_c as oc
from tests.test_gpu_stats import model_histogram
from tests.util import ESA_NASTY, HSG_NASTY

pytestmark = pytest.mark.gpu

K1 = 3                      # the table of the single-raster launches
HIST_BYTES = 16 * 256 * 8


def clamp_columns(ci, hsx):
    """The column rule of prepare_tile: (uint32) ci < hsx ? ci : hsx - 1, whatever the value."""
    u = np.asarray(ci, np.int32).view(np.uint32).astype(np.int64)
    return np.where(u < hsx, u, hsx - 1)


class Tile:
    """One landcover strip, soil window and index maps on the device, and what the oracle makes of them."""

    def __init__(self, eng, tables, seed, W, H, hsx, hsy, ci=None, cj=None):
        rng = np.random.default_rng(seed)
        self.eng, self.W, self.H, self.hsx, self.hsy = eng, W, H, hsx, hsy
        self.esa = rng.choice(ESA_NASTY, size=(H, W)).astype(np.uint8)
        self.coarse = rng.choice(HSG_NASTY, size=(hsy, hsx)).astype(np.uint8)
        self.ci = (np.arange(W) * hsx // W).astype(np.int32) if ci is None else np.asarray(ci, np.int32)
        # rows of soil that do not start with a strip: 13-row strips begin inside a soil row
        self.cj = np.minimum((np.arange(H) + 3) * hsy // (H + 3), hsy - 1).astype(np.int32) if cj is None else cj
        self.soil = self.coarse[self.cj][:, clamp_columns(self.ci, hsx)]
        self.tables, self._want, self._soil = tables, {}, {}
        self.bufs = self.upload_inputs()
        self.outs = {}

    def upload_inputs(self):
        return [self.eng.upload(a) for a in (self.esa, self.coarse, self.ci, self.cj)]

    def prepare(self, stream=None):
        self.eng.prepare_tile(self.bufs[1].ptr, self.hsx, self.hsy, self.bufs[2].ptr, self.W, stream)

    def want(self, r):
        """Raster r = condition * 9 + table as the oracle computes it (computed once, kept)."""
        if r not in self._want:
            c = r // 9
            if c not in self._soil:
                self._soil[c] = oc.modify_hysogs_data(self.soil, c == 0)
            self._want[r] = oc.calculate_cn(self.esa, self._soil[c], self.tables[r % 9]).reshape(self.H, self.W)
        return self._want[r]

    def out(self, r):
        if r not in self.outs:
            self.outs[r] = self.eng.alloc(self.W * self.H)
        return self.outs[r]

    def launch(self, cond_mask, table_mask, strip_rows=None, stream=None):
        """Strips over the whole tile into poisoned rasters; the rasters written."""
        sel = [c * 9 + k for c in range(2) for k in range(9) if cond_mask >> c & 1 and table_mask >> k & 1]
        for r in sel:
            self.eng.memset(self.out(r).ptr, 0xA5, self.W * self.H, stream)
        step = strip_rows or self.H
        for y0 in range(0, self.H, step):
            rows = min(step, self.H - y0)
            ptrs = [self.out(r).at(y0 * self.W) if r in sel else None for r in range(18)]
            self.eng.cn_strip(self.bufs[0].at(y0 * self.W), self.W, rows, self.bufs[3].at(4 * y0), cond_mask,
                              table_mask, ptrs, stream)
        return sel

    def check(self, rasters, what, stream=None):
        self.eng.sync(stream)
        for r in rasters:
            got = self.eng.download(self.outs[r].ptr, (self.H, self.W))
            bad = np.flatnonzero(got != self.want(r))
            assert bad.size == 0, "%s: raster %d differs in %d pixels, first at %d" % (what, r, bad.size, bad[0])

    def run(self, cond_mask, table_mask, what, strip_rows=None):
        self.check(self.launch(cond_mask, table_mask, strip_rows), what)

    def histogram(self, stream=None):
        hist = self.eng.alloc(HIST_BYTES)
        try:
            self.eng.memset(hist.ptr, 0, HIST_BYTES, stream)
            self.eng.pair_histogram(self.bufs[0].ptr, self.W, self.H, self.bufs[3].ptr, hist.ptr, stream)
            return self.eng.download(hist.ptr, (16 * 256,), np.uint64, stream)
        finally:
            hist.close()

    def close(self):
        for b in self.bufs + list(self.outs.values()):
            b.close()


@pytest.fixture
def eng9(engine, tables):
    engine.set_tables(tables)
    yield engine
    engine.set_option("defaults", 0)


def test_a_the_tables_are_a_snapshot_of_the_callers_buffers(eng9, tables):
    """Case A: after prepare_tile nothing reads the caller's coarse and ci, neither the strips of the compact words nor
    the code bytes made later for a byte strip and for the pair histogram."""
    t = Tile(eng9, tables, 1, 2048, 24, 90, 6)
    try:
        t.prepare()
        eng9.sync()
        eng9.memset(t.bufs[1].ptr, 0xEE, t.coarse.nbytes)
        eng9.memset(t.bufs[2].ptr, 0xEE, t.ci.nbytes)
        eng9.sync()
        assert eng9.soil_words_state() == 1
        t.run(3, 1 << K1, "tables, one table")
        t.run(3, 0x1ff, "tables, all tables")
        eng9.set_option("compact_soil", 0)
        t.run(3, 1 << K1, "bytes made after the caller's buffers were overwritten")
        np.testing.assert_array_equal(t.histogram(), model_histogram(t.esa, t.soil))
    finally:
        t.close()


@pytest.mark.parametrize("W,H,hsx,hsy", [(1040, 40, 50, 5), (4112, 21, 170, 3)])
def test_b_option_switched_between_strips_of_one_prepared_tile(eng9, tables, W, H, hsx, hsy):
    """Case B, the benchmark's sequence: a strip of the tables, then compact_soil = 0 and a strip with NO new
    prepare_tile (the bytes are made for it), then the option back on and a strip."""
    t = Tile(eng9, tables, W, W, H, hsx, hsy)
    try:
        t.prepare()
        t.run(1, 1 << K1, "tables")
        eng9.set_option("compact_soil", 0)
        t.run(1, 1 << K1, "bytes, no new prepare_tile")
        t.run(3, 0x1ff, "bytes, all tables")
        eng9.set_option("compact_soil", 1)
        t.run(1, 1 << K1, "tables again")
        t.run(3, 0x1ff, "tables again, all tables")
    finally:
        t.close()


@pytest.mark.parametrize("first", ["strip", "histogram"])
def test_c_two_streams_share_the_bytes_of_one_prepared_tile(eng9, tables, first):
    """Case C: prepare_tile on one stream, then a byte strip on a second and the pair histogram on a third, both
    ordered after prepare_tile by an event only: whichever comes second waits for the bytes the first one made."""
    t = Tile(eng9, tables, 7, 2048, 24, 90, 6)
    s1, s2, ev = eng9.stream_create(), eng9.stream_create(), eng9.event_create()
    try:
        t.prepare()
        eng9.event_record(ev)
        eng9.stream_wait_event(s1, ev)
        eng9.stream_wait_event(s2, ev)
        eng9.set_option("compact_soil", 0)      # after prepare_tile: the bytes are not made yet
        if first == "strip":
            rasters = t.launch(3, 1 << K1, stream=s1)
            hist = t.histogram(s2)
        else:
            hist = t.histogram(s2)
            rasters = t.launch(3, 1 << K1, stream=s1)
        t.check(rasters, "byte strip on its own stream", s1)
        np.testing.assert_array_equal(hist, model_histogram(t.esa, t.soil))
    finally:
        eng9.sync(s1)
        eng9.sync(s2)
        eng9.stream_destroy(s1)
        eng9.stream_destroy(s2)
        eng9.event_destroy(ev)
        t.close()


def _with_complex_group(W, hsx, g):
    """A map of wide soil cells whose only group with more than two runs is group g."""
    ci = (np.arange(W) * hsx // W).astype(np.int32)
    n = min(16, W - 16 * g)
    assert n >= 3
    ci[16 * g:16 * g + n] = ci[16 * g]
    ci[16 * g + 1] = (ci[16 * g] + 2) % hsx         # a, b, a ...: three runs
    return ci


@pytest.mark.parametrize("W,group", [(2048, 0), (2048, 127), (2064, 64), (2051, 128)],
                         ids=["first", "last", "middle", "holds-column-W-1"])
def test_d_one_complex_group_makes_the_tile_complex(eng9, tables, W, group):
    """Case D: the flag is raised wherever the only complex group lies (2051: the group that holds column W-1 is
    not a whole one), and the strips of such a tile are right: one table and all tables, whole and in 13-row
    strips that start inside a soil row."""
    t = Tile(eng9, tables, W + group, W, 40, 64, 5, ci=_with_complex_group(W, 64, group))
    try:
        t.prepare()
        assert eng9.soil_words_state() == 2
        t.run(3, 1 << K1, "one table")
        t.run(3, 0x1ff, "all tables")
        t.run(3, 1 << K1, "one table, 13-row strips", strip_rows=13)
        t.run(3, 0x1ff, "all tables, 13-row strips", strip_rows=13)
    finally:
        t.close()


@pytest.mark.parametrize("hsx,hsy", [(1, 1), (1, 4), (70, 1)])
def test_d_one_soil_column_or_row(eng9, tables, hsx, hsy):
    """Case D: hsx = 1 (the codes table is one column and its padding), hsy = 1 (one soil row for every strip)."""
    t = Tile(eng9, tables, hsx * 10 + hsy, 2048, 40, hsx, hsy)
    try:
        t.prepare()
        assert eng9.soil_words_state() == 1
        t.run(3, 1 << K1, "one table")
        t.run(3, 0x1ff, "all tables")
        t.run(3, 1 << K1, "one table, 13-row strips", strip_rows=13)
        t.run(3, 0x1ff, "all tables, 13-row strips", strip_rows=13)
        eng9.set_option("compact_soil", 0)
        t.run(3, 1 << K1, "bytes")
    finally:
        t.close()


@pytest.mark.parametrize("kind,state", [("runs", 1), ("scattered", 2)])
def test_e_columns_outside_the_window_are_clamped_unsigned(eng9, tables, kind, state):
    """Case E: negative ci and ci >= hsx name column hsx - 1, in the tables and in the bytes.  "runs": whole
    groups of such values at both ends (every group stays compact); "scattered": single ones anywhere."""
    W, hsx = 2048, 64
    ci = (np.arange(W) * hsx // W).astype(np.int32)
    outside = np.array([-1, -5, hsx, hsx + 7, 2 ** 31 - 1, -2 ** 31, 1 << 24, -(1 << 24)], np.int32)
    if kind == "runs":
        ci[:32] = np.repeat(outside[:2], 16)
        ci[-48:] = np.repeat(outside[2:5], 16)
    else:
        at = np.random.default_rng(3).choice(W, size=200, replace=False)
        ci[at] = outside[np.arange(200) % outside.size]
        ci[0], ci[W - 1] = -1, hsx
    t = Tile(eng9, tables, 11, W, 24, hsx, 6, ci=ci)
    try:
        t.prepare()
        assert eng9.soil_words_state() == state
        t.run(3, 1 << K1, "tables, one table")
        t.run(3, 0x1ff, "tables, all tables")
        eng9.set_option("compact_soil", 0)
        t.run(3, 1 << K1, "bytes, one table")
        np.testing.assert_array_equal(t.histogram(), model_histogram(t.esa, t.soil))
    finally:
        t.close()


def test_f_aligned_strips_take_every_pixel_from_the_tables(eng9, tables):
    """Case F: strips of a W % 16 == 0 tile, at pointer offsets inside the rasters, take every pixel -- the last
    ones of a strip included -- from the tables.  W % 16 == 0 makes the pixel count of every strip a multiple of
    16, so the byte-wise tail of the vector kernels has no pixels in such a strip, and such a launch carries no
    pointer to the byte workspace at all (a read of it would fault, not miscompute): what results can show is
    that every pixel of every strip is right and that the tile stays in state 1."""
    t = Tile(eng9, tables, 22, 2048, 40, 90, 6)
    try:
        t.prepare()
        for rows in (13, 1, 7):
            t.run(3, 1 << K1, "one table, %d-row strips" % rows, strip_rows=rows)
            t.run(3, 0x1ff, "all tables, %d-row strips" % rows, strip_rows=rows)
        assert eng9.soil_words_state() == 1
    finally:
        t.close()


@pytest.mark.parametrize("complex_tile", [False, True])
def test_several_trips_per_wave(eng9, tables, complex_tile):
    """8 M pixels on one workgroup per CU: 2048 chunks on 256 workgroups, so every wave runs 2 to 8 trips -- without
    and with the software pipeline's two register sets, one, two and four chunks per trip, one raster and all 18,
    from the compact words and (complex tile) pixel by pixel from the codes table."""
    W, H, hsx = 2048, 4096, 90
    ci = _with_complex_group(W, hsx, 5) if complex_tile else None
    t = Tile(eng9, tables, 31, W, H, hsx, 160, ci=ci)
    try:
        t.prepare()
        assert eng9.soil_words_state() == (2 if complex_tile else 1)
        eng9.set_option("grid_blocks_per_cu", 1)
        for ilp1, pf in ((1, 0), (1, 1), (2, 1), (4, 0)):
            eng9.set_option("ilp1", ilp1)
            eng9.set_option("prefetch", pf)
            t.run(1, 1 << K1, "one raster, ilp %d, pipeline %d" % (ilp1, pf))
        for ilp16, pf in ((1, 1), (2, 0)):
            eng9.set_option("ilp16", ilp16)
            eng9.set_option("prefetch", pf)
            t.run(3, 0x1ff, "all tables, ilp %d, pipeline %d" % (ilp16, pf))
    finally:
        t.close()
