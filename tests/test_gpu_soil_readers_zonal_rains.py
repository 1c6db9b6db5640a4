"""GPU: gcn10_gpu_zonal_sums_rains, one more reader of the code bytes of a prepared tile, held to the tiles and sequences
A to I and to the second-stream case exactly as tests/test_gpu_soil_readers_zonal_rain.py holds the one-raster call: the
spans of soil_readers.reader_spans, cut by k = 3 random fields of 13 x 5 px cells (gcn10_zone_rains_cut) and summed with
256 tables.  On every tile the reader is the first call after a prepare_tile of its own.  Needs an MI355X.

Expected values: the oracle's rasters summed over the cut spans with the tables of every item's tuple in numpy -- never
another GPU path.
"""
import numpy as np
import pytest

from gcn10_amd import host
from tests import rainutil as rn
from tests import soil_readers as sr
from tests.soil_readers import SPECS, make_tile, run_reader
from tests.test_gpu_soil_readers import _other_soil, eng9  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

TABLES = rn.tables_256()
TILES_A_TO_F = [k for k in SPECS if k[0] in "ABCDEF"]
TILES_G = [k for k in SPECS if k[0] == "G"]
GUARD = 64
K = 3


class ZonalRainsReader(sr.Reader):
    name = "zonal, rains"

    def __init__(self, tile):
        super().__init__(tile)
        t = tile
        self.eng.set_rain_tables(TABLES)
        cellx, celly = (np.arange(t.W) // 13).astype(np.int32), (np.arange(t.H) // 5).astype(np.int32)
        fields = np.random.default_rng(t.W * 7 + t.H).integers(0, 256, (K, int(celly.max()) + 1, int(cellx.max()) + 1))
        fields[1] = fields[1] // 128 * 77                # a layer of two bytes: tuples that share it
        self.cut = host.zone_rains_cut({"spans": sr.reader_spans(t.W, t.H)}, t.W, t.H,
                                       {"cellx": cellx, "celly": celly, "cx0": 0, "cy0": 0}, fields.astype(np.uint8),
                                       n_local=2)
        s2, items = self.cut["spans"], self.cut["items"]
        assert ((s2["y"] >= 0) & (s2["y"] < t.H) & (s2["x0"] >= 0) & (s2["x0"] < s2["x1"]) & (s2["x1"] <= t.W) &
                (s2["zone"] >= 0) & (s2["zone"] < 2)).all()
        assert int(items["n_spans"].sum()) == s2.size and int(items["first_span"][-1] + items["n_spans"][-1]) == s2.size
        self.n_items = items.size
        self.dev = [self.upload(s2), self.upload(items)]
        self.nbytes = 2 * 18 * (2 + K) * 8
        self.out = self.alloc(self.nbytes + 2 * GUARD)

    def launch(self, stream=None):
        t = self.t
        self.eng.memset(self.out.ptr, 0xA5, self.nbytes + 2 * GUARD, stream)
        self.eng.memset(self.out.at(GUARD), 0, self.nbytes, stream)
        self.eng.zonal_sums_rains_device(self.esa.ptr, t.W, t.H, self.cj.ptr, self.dev[0].ptr, self.dev[1].ptr,
                                         self.n_items, 2, 3, 0x1FF, K, self.out.at(GUARD), stream)

    def check(self):
        t = self.t
        img = self.eng.download(self.out.ptr, (self.nbytes + 2 * GUARD,))
        assert (img[:GUARD] == 0xA5).all() and (img[GUARD + self.nbytes:] == 0xA5).all(), \
            "zonal rains: a byte outside the words was written"
        got = img[GUARD:GUARD + self.nbytes].view(np.uint64).astype(np.int64).reshape(2, 18, 2 + K)
        spans, items = self.cut["spans"], self.cut["items"]
        tab = TABLES.astype(np.int64)
        length = (spans["x1"] - spans["x0"]).astype(np.int64)
        ys, zs = (np.repeat(a.astype(np.int64), length) for a in (spans["y"], spans["zone"]))
        ts = [np.repeat(np.repeat(items["table"][:, j].astype(np.int64), items["n_spans"].astype(np.int64)), length)
              for j in range(K)]
        xs = np.concatenate([np.arange(a, b, dtype=np.int64) for a, b in zip(spans["x0"], spans["x1"])])
        want = np.zeros((2, 18, 2 + K), np.int64)
        for r in range(18):
            v = t.want(r)[ys, xs].astype(np.int64)
            ok = v != 255
            words = [v[ok], np.ones(int(ok.sum()), np.int64)] + [tab[ts[j][ok], v[ok]] for j in range(K)]
            for word, w in enumerate(words):
                np.add.at(want[:, r, word], zs[ok], w)
        bad = np.argwhere(got != want).tolist()
        at = tuple(bad[0]) if bad else None
        assert not bad, "zonal rains: %d of %d words differ, first at (zone, raster, word) = %s: got %d, want %d" % (
            len(bad), want.size, at, got[at], want[at])


@pytest.mark.parametrize("name", TILES_A_TO_F)
def test_tiles_a_to_f(eng9, tables, name):  # noqa: F811
    t = make_tile(eng9, tables, name)
    try:
        t.prepare()
        run_reader(t, ZonalRainsReader)
    finally:
        eng9.sync()
        t.close()


@pytest.mark.parametrize("name", TILES_G)
def test_g_pointers_as_the_abi_allows_them(eng9, tables, name):  # noqa: F811
    """The pointers of case G, after an aligned tile of other soil, as in tests/test_gpu_soil_readers.py."""
    aligned = _other_soil(eng9, tables, name)
    shifted = None
    try:
        aligned.prepare()
        shifted = make_tile(eng9, tables, name, offsets=sr.SHIFTED)
        assert shifted.bufs[2].ptr % 16 == 4 and shifted.bufs[0].ptr % 4 == 3
        shifted.prepare()
        run_reader(shifted, ZonalRainsReader)
    finally:
        eng9.sync()
        aligned.close()
        if shifted is not None:
            shifted.close()


@pytest.mark.parametrize("name", ["A-zig-zag", "G-2048"])
def test_h_the_prepared_soil_is_a_snapshot(eng9, tables, name):  # noqa: F811
    t = make_tile(eng9, tables, name)
    try:
        t.prepare()
        eng9.sync()
        eng9.memset(t.bufs[1].ptr, 0xEE, t.coarse.nbytes)
        eng9.memset(t.bufs[2].ptr, 0xEE, t.ci.nbytes)
        eng9.sync()
        run_reader(t, ZonalRainsReader)
    finally:
        eng9.sync()
        t.close()


def test_i_tile_after_tile_on_one_context(eng9, tables):  # noqa: F811
    """Tile 1 with the reader run, so that its bytes are in the workspace; then a smaller tile and a third as large as
    the first with other soil: on each the reader is the first call after prepare_tile."""
    tiles = []
    try:
        for spec in sr.CASE_I:
            tiles.append(sr.ReaderTile(eng9, tables, key="I-%d" % spec["seed"], **spec))
        for t in tiles:
            t.prepare()
            run_reader(t, ZonalRainsReader)
    finally:
        eng9.sync()
        for t in tiles:
            t.close()


@pytest.mark.parametrize("W", [2048, 2051])
@pytest.mark.parametrize("other", ["strip", "zonal"])
def test_beside_another_reader_on_a_second_stream(eng9, tables, other, W):  # noqa: F811
    """prepare_tile on the main stream, an event, two side streams that wait for it: this reader on one, `other` on the
    other, either way round; nothing else orders them, and both results are checked."""
    t = sr.ReaderTile(eng9, tables, 3100 + W % 2 + 2 * (other == "zonal"), W, 40, 90, 6)
    s1 = s2 = ev = None
    rd = []
    try:
        s1, s2, ev = eng9.stream_create(), eng9.stream_create(), eng9.event_create()
        for first, second in ((ZonalRainsReader, sr.READER_CLASSES[other]), (sr.READER_CLASSES[other], ZonalRainsReader)):
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
