"""GPU: gcn10_gpu_grid_sums_rain, the ninth reader of the code bytes of a prepared tile, held to the tiles and sequences
A to I the way tests/test_gpu_soil_readers.py holds the grid reader: the passes of soil_readers.grid_passes (cells of
8 px of one row over the whole tile; cells of 25 x 25.6 px with -1 around them in the two strips that start inside a
soil row), both through the rain call with a random byte per cell and 256 tables.  On every tile the reader is the
first call after a prepare_tile of its own.  Needs an MI355X.

Expected values: the oracle's rasters summed per cell with the cell's table in numpy (tests/rainutil.py) -- never
another GPU path.
"""
import numpy as np
import pytest

from tests import rainutil as rn
from tests import soil_readers as sr
from tests.soil_readers import SPECS, make_tile, run_reader
from tests.test_gpu_soil_readers import _other_soil, eng9  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

TABLES = rn.tables_256()
TILES_A_TO_F = [k for k in SPECS if k[0] in "ABCDEF"]
TILES_G = [k for k in SPECS if k[0] == "G"]


class RainGridReader(sr.GridReader):
    """The passes of the grid reader as triples with a table per cell.  set_rain_tables is synchronous and independent
    of every other table of the context, so two of these readers do not disturb each other."""
    name = "grid, rain"

    def set_weights_and_passes(self):
        t = self.t
        self.eng.set_rain_tables(TABLES)
        passes = sr.grid_passes(t.W, t.H, t.cj)
        for i, p in enumerate(passes):
            p.update(call="grid_sums_rain", words=3,
                     field=np.random.default_rng(40 + i).integers(0, 256, (p["ncy"], p["ncx"])).astype(np.uint8))
        return passes

    def launch(self, stream=None):
        t = self.t
        self.eng.memset(self.out.ptr, 0xA5, self.total, stream)
        for p in self.passes:
            if "field_dev" not in p:
                p["field_dev"] = self.upload(p["field"])
            self.eng.memset(self.out.at(p["off"]), 0, p["nbytes"], stream)
            for y0, rows in p["strips"]:
                self.eng.grid_sums_rain(self.esa.at(y0 * t.W), t.W, rows, self.cj.at(4 * y0), p["dev"][0].ptr,
                                        p["dev"][1].at(4 * y0), p["ncx"], p["ncy"], p["masks"][0], p["masks"][1],
                                        p["field_dev"].ptr, self.out.at(p["off"]), stream)

    def check(self):
        t = self.t
        got = self.eng.download(self.out.ptr, (self.total,))
        poison = np.ones(self.total, bool)
        for p in self.passes:
            poison[p["off"]:p["off"] + p["nbytes"]] = False
            want = np.zeros((len(p["sel"]), p["ncy"], p["ncx"], 3), np.int64)
            for q, r in enumerate(p["sel"]):
                for y0, rows in p["strips"]:
                    rn.add_triples(want[q], t.want(r)[y0:y0 + rows], p["cellx"], p["celly"][y0:y0 + rows], p["field"],
                                   TABLES)
            words = got[p["off"]:p["off"] + p["nbytes"]].view(np.uint64).astype(np.int64).reshape(want.shape)
            bad = np.argwhere(words != want).tolist()
            at = tuple(bad[0]) if bad else None
            assert not bad, "rain pass '%s' in %d strips: %d of %d words differ, first in raster %d at (cell row, cell, " \
                "word) = %s: got %d, want %d" % (p["name"], len(p["strips"]), len(bad), want.size, p["sel"][at[0]],
                                                 at[1:], words[at], want[at])
        assert (got[poison] == 0xA5).all(), "rain: a byte outside the words was written"


@pytest.mark.parametrize("name", TILES_A_TO_F)
def test_tiles_a_to_f(eng9, tables, name):
    t = make_tile(eng9, tables, name)
    try:
        t.prepare()
        run_reader(t, RainGridReader)
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
        run_reader(shifted, RainGridReader)
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
        run_reader(t, RainGridReader)
    finally:
        eng9.sync()
        t.close()


def test_i_tile_after_tile_on_one_context(eng9, tables):
    """Tile 1 with the rain reader run, so that its bytes are in the workspace; then a smaller tile and a third as large
    as the first with other soil: on each the rain reader is the first call after prepare_tile."""
    tiles = []
    try:
        for spec in sr.CASE_I:
            tiles.append(sr.ReaderTile(eng9, tables, key="I-%d" % spec["seed"], **spec))
        for t in tiles:
            t.prepare()
            run_reader(t, RainGridReader)
    finally:
        eng9.sync()
        for t in tiles:
            t.close()


@pytest.mark.parametrize("W", [2048, 2051])
@pytest.mark.parametrize("other", ["strip", "grid"])
def test_beside_another_reader_on_a_second_stream(eng9, tables, other, W):
    """prepare_tile on the main stream, an event, two side streams that wait for it: the rain reader on one, `other` on
    the other, either way round; nothing else orders them, and both results are checked."""
    t = sr.ReaderTile(eng9, tables, 3000 + W % 2 + 2 * (other == "grid"), W, 40, 90, 6)
    s1 = s2 = ev = None
    rd = []
    try:
        s1, s2, ev = eng9.stream_create(), eng9.stream_create(), eng9.event_create()
        for first, second in ((RainGridReader, sr.READER_CLASSES[other]), (sr.READER_CLASSES[other], RainGridReader)):
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
