"""GPU: gcn10_gpu_runoff_strip, the eleventh reader of the code bytes of a prepared tile, held to the tiles and sequences
A to I the way tests/test_gpu_soil_readers_rain.py holds the rain sums: all 18 rasters in one call over the whole tile
under cells of 37.3 px with -1 runs and 256 random tables, then a subset of the rasters in the two strips that start inside
a soil row, under cells of 16 px x 3 rows.  On every tile the reader is the first call after a prepare_tile of its own.
Needs an MI355X.

Expected values: T[table of the pixel's cell][value of the oracle's raster] in numpy (test_gpu_runoff_strip.want_raster)
-- never another GPU path.
"""
import numpy as np
import pytest

from tests import soil_readers as sr
from tests.soil_readers import SPECS, make_tile, run_reader
from tests.test_gpu_runoff_strip import GUARD, POISON, cell_map, random_tables, want_raster
from tests.test_gpu_soil_readers import _other_soil, eng9  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

TABLES = random_tables(256, seed=90)
TILES_A_TO_F = [k for k in SPECS if k[0] in "ABCDEF"]
TILES_G = [k for k in SPECS if k[0] == "G"]


class RunoffStripReader(sr.Reader):
    """Two passes into poisoned rasters between guard bytes.  set_cell_byte_tables is synchronous and independent of
    every other table of the context, so the reader does not disturb another one."""
    name = "runoff strip"

    def __init__(self, tile):
        super().__init__(tile)
        t = tile
        self.eng.set_cell_byte_tables(TABLES)
        self.n = t.W * t.H
        self.slot = (GUARD + self.n + GUARD + 255) & ~255
        self.passes = [dict(x="edges", y="3", masks=(3, 0x1FF), strips=[(0, t.H)]),
                       dict(x="16", y="3", masks=(2, 0x0A1), strips=sr.strips_inside_a_soil_row(t.cj))]
        self.total = 0
        for i, p in enumerate(self.passes):
            (p["cellx"], p["ncx"]), (p["celly"], p["ncy"]) = cell_map(p["x"], t.W), cell_map(p["y"], t.H)
            p["field"] = np.random.default_rng(60 + i).integers(0, 256, (p["ncy"], p["ncx"])).astype(np.uint8)
            p["dev"] = [self.upload(a) for a in (p["cellx"], p["celly"], p["field"])]
            p["sel"] = sr.selected(*p["masks"])
            p["off"] = self.total
            self.total += len(p["sel"]) * self.slot
        self.out = self.alloc(self.total)

    def launch(self, stream=None):
        t = self.t
        self.eng.memset(self.out.ptr, POISON, self.total, stream)
        for p in self.passes:
            at = {r: p["off"] + q * self.slot + GUARD for q, r in enumerate(p["sel"])}
            for y0, rows in p["strips"]:
                ptrs = [self.out.at(at[r] + y0 * t.W) if r in at else None for r in range(18)]
                self.eng.runoff_strip(self.esa.at(y0 * t.W), t.W, rows, self.cj.at(4 * y0), p["dev"][0].ptr,
                                      p["dev"][1].at(4 * y0), p["ncx"], p["ncy"], p["dev"][2].ptr, p["masks"][0],
                                      p["masks"][1], ptrs, stream)

    def check(self):
        t = self.t
        got = self.eng.download(self.out.ptr, (self.total,))
        poison = np.ones(self.total, bool)
        for i, p in enumerate(self.passes):
            for q, r in enumerate(p["sel"]):
                a = p["off"] + q * self.slot + GUARD
                poison[a:a + self.n] = False
                want = want_raster(t.want(r), p["cellx"], p["celly"], p["ncx"], p["ncy"], p["field"], TABLES)
                bad = np.argwhere(got[a:a + self.n].reshape(t.H, t.W) != want)
                assert bad.size == 0, "runoff strip pass %d in %d strips, raster %d: %d pixels differ, first at %s" % (
                    i, len(p["strips"]), r, len(bad), tuple(bad[0]))
        assert (got[poison] == POISON).all(), "runoff strip: a byte outside the rasters was written"


@pytest.mark.parametrize("name", TILES_A_TO_F)
def test_tiles_a_to_f(eng9, tables, name):
    t = make_tile(eng9, tables, name)
    try:
        t.prepare()
        run_reader(t, RunoffStripReader)
    finally:
        eng9.sync()
        t.close()


@pytest.mark.parametrize("name", TILES_G)
def test_g_pointers_as_the_abi_allows_them(eng9, tables, name):
    """The pointers of case G, after an aligned tile of other soil, as in tests/test_gpu_soil_readers.py."""
    aligned = _other_soil(eng9, tables, name)
    shifted = None
    try:
        aligned.prepare()
        shifted = make_tile(eng9, tables, name, offsets=sr.SHIFTED)
        assert shifted.bufs[2].ptr % 16 == 4 and shifted.bufs[0].ptr % 4 == 3
        shifted.prepare()
        run_reader(shifted, RunoffStripReader)
    finally:
        eng9.sync()
        aligned.close()
        if shifted is not None:
            shifted.close()


@pytest.mark.parametrize("name", ["A-zig-zag", "G-2048"])
def test_h_the_prepared_soil_is_a_snapshot(eng9, tables, name):
    t = make_tile(eng9, tables, name)
    try:
        t.prepare()
        eng9.sync()
        eng9.memset(t.bufs[1].ptr, 0xEE, t.coarse.nbytes)
        eng9.memset(t.bufs[2].ptr, 0xEE, t.ci.nbytes)
        eng9.sync()
        run_reader(t, RunoffStripReader)
    finally:
        eng9.sync()
        t.close()


def test_i_tile_after_tile_on_one_context(eng9, tables):
    """Tile 1 with the reader run, so that its bytes are in the workspace; then a smaller tile and a third as large as the
    first with other soil: on each the reader is the first call after prepare_tile."""
    tiles = []
    try:
        for spec in sr.CASE_I:
            tiles.append(sr.ReaderTile(eng9, tables, key="I-%d" % spec["seed"], **spec))
        for t in tiles:
            t.prepare()
            run_reader(t, RunoffStripReader)
    finally:
        eng9.sync()
        for t in tiles:
            t.close()


@pytest.mark.parametrize("W", [2048, 2051])
@pytest.mark.parametrize("other", ["strip", "grid"])
def test_beside_another_reader_on_a_second_stream(eng9, tables, other, W):
    """prepare_tile on the main stream, an event, two side streams that wait for it: this reader on one, `other` on the
    other, either way round; nothing else orders them, and both results are checked."""
    t = sr.ReaderTile(eng9, tables, 3000 + W % 2 + 2 * (other == "grid"), W, 40, 90, 6)
    s1 = s2 = ev = None
    rd = []
    try:
        s1, s2, ev = eng9.stream_create(), eng9.stream_create(), eng9.event_create()
        for first, second in ((RunoffStripReader, sr.READER_CLASSES[other]), (sr.READER_CLASSES[other], RunoffStripReader)):
            pair = [first(t), second(t)]
            rd += pair
            t.prepare()
            eng9.event_record(ev)
            eng9.stream_wait_event(s1, ev)
            eng9.stream_wait_event(s2, ev)
            pair[0].launch(s1)
            pair[1].launch(s2)
            eng9.sync(s1)
            eng9.sync(s2)
            pair[0].check()
            pair[1].check()
    finally:
        for s in (s1, s2):
            if s is not None:
                eng9.sync(s)
                eng9.stream_destroy(s)
        if ev is not None:
            eng9.event_destroy(ev)
        for r in rd:
            r.close()
        t.close()
