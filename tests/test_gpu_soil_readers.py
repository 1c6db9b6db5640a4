"""GPU: every reader of the code bytes of a prepared tile -- the byte and vector strip kernels, the fused tile
encoder, verify_strip, the pair histogram, the zonal pair histogram, the average overviews, the area means of
gcn10_gpu_aggregate and the sums on a model grid of gcn10_gpu_grid_sums / _storms (eight readers,
tests/soil_readers.READERS; the three-word gcn10_gpu_grid_sums_weighted in a test of its own) -- held to the contract
of gcn10_gpu_prepare_tile in include/gcn10_gpu.h, on the tiles A to I where that machinery can go wrong: column maps that are not monotone
or leave the window, one complex group, one soil column or row, cells narrower than a pixel, widths around the 16-px group, two tile rows, pointers at odd offsets, the caller's buffers overwritten after
prepare_tile, and tile after tile on one context.  On every tile every reader is the first call after a
prepare_tile of its own, so it is the one that makes the bytes (or, where the width is no multiple of 16, waits
for the ones prepare_tile made).  Needs an MI355X.

Expected values: the oracle's calculate_cn / modify_hysogs_data over coarse[cj][:, clamp_columns(ci, hsx)] by plain
numpy indexing, numpy pair counts, the numpy model of the average overviews, the numpy reduction of the oracle's
rasters to cells and their int64 sums over the maps of a model grid (tests/soil_readers.py, whose references
tests/test_soil_reader_references.py checks on the CPU) -- never another GPU path.
"""
import numpy as np
import pytest

from tests import soil_readers as sr
from tests.soil_readers import READERS, SPECS, make_tile, run_reader

pytestmark = pytest.mark.gpu

TILES_A_TO_F = [k for k in SPECS if k[0] in "ABCDEF"]
TILES_G = [k for k in SPECS if k[0] == "G"]


@pytest.fixture
def eng9(engine, tables):
    engine.set_tables(tables)
    engine.set_option("defaults", 0)
    yield engine
    engine.set_option("defaults", 0)


@pytest.mark.parametrize("name", TILES_A_TO_F)
@pytest.mark.parametrize("reader", READERS)
def test_tiles_a_to_f(eng9, tables, reader, name):
    """Cases A to F: the reader is the first call after prepare_tile.  (The tile varies fastest, so the bytes the
    test before left in the workspace are another tile's.)"""
    t = make_tile(eng9, tables, name)
    try:
        t.prepare()
        run_reader(t, reader)
    finally:
        eng9.sync()
        t.close()


def _other_soil(eng, tables, name):
    """The tile `name` with the same maps and shape, other landcover and soil, uploaded aligned."""
    spec = dict(SPECS[name], seed=SPECS[name]["seed"] + 1000)
    return sr.ReaderTile(eng, tables, **spec)


@pytest.mark.parametrize("name", TILES_G)
@pytest.mark.parametrize("reader", READERS)
def test_g_pointers_as_the_abi_allows_them(eng9, tables, reader, name):
    """Case G: ci at byte offset 4 of its buffer (soil_tables_kernel<false>: no 16-byte loads of the map), coarse at
    offset 1, the landcover at offset 3.  The tile is in the state the aligned upload of the same maps gives, and every
    reader sees its soil.  The aligned tile has OTHER soil, so that at W = 2051, where prepare_tile makes the bytes
    itself, the ones it left in the workspace are wrong for the shifted tile."""
    aligned = _other_soil(eng9, tables, name)
    shifted = None
    try:
        aligned.prepare()
        state = eng9.soil_words_state()
        shifted = make_tile(eng9, tables, name, offsets=sr.SHIFTED)
        assert shifted.bufs[2].ptr % 16 == 4 and shifted.bufs[1].ptr % 2 == 1 and shifted.bufs[0].ptr % 4 == 3
        assert np.array_equal(shifted.ci, aligned.ci) and (shifted.soil != aligned.soil).mean() > 0.5
        shifted.prepare()
        assert eng9.soil_words_state() == state
        run_reader(shifted, reader)
    finally:
        eng9.sync()
        aligned.close()
        if shifted is not None:
            shifted.close()


@pytest.mark.parametrize("name", TILES_A_TO_F + TILES_G)
def test_the_weighted_grid_sums_on_tiles_a_to_g(eng9, tables, name):
    """gcn10_gpu_grid_sums_weighted, the kernel of three words per cell: a context holds one weight table or several,
    so it cannot be one of READERS beside the k = 2 of the grid reader.  set_weights("random"), then the `rows` pass as
    the first call after prepare_tile, exact against the oracle's rasters summed with one table.  G: the pointers of
    case G, after an aligned tile of other soil as there."""
    aligned = _other_soil(eng9, tables, name) if name in TILES_G else None
    t = None
    try:
        if aligned is not None:
            aligned.prepare()
        t = make_tile(eng9, tables, name, offsets=sr.SHIFTED if name in TILES_G else None)
        t.prepare()
        run_reader(t, sr.WeightedGridReader)
    finally:
        eng9.sync()
        for tile in (aligned, t):
            if tile is not None:
                tile.close()


@pytest.mark.parametrize("name,state", [("G-2048", 1), ("A-decreasing", 1), ("B-runs", 1), ("A-zig-zag", 2),
                                        ("C-last", 2)])
def test_g_compact_words_from_a_map_that_is_not_16_byte_aligned(eng9, tables, name, state):
    """Case G, what soil_tables_kernel<false> writes besides the column map and the codes: the compact words and the
    complex flag.  ci at byte offset 4 and coarse at offset 1 again, but the landcover aligned, so that the strips of
    this W % 16 == 0 tile read the words (state 1) or go through codes and cx pixel by pixel (state 2) -- never the
    code bytes.  The tile prepared before has the same maps and other soil."""
    aligned = _other_soil(eng9, tables, name)
    shifted = None
    try:
        aligned.prepare()
        assert eng9.soil_words_state() == state
        shifted = make_tile(eng9, tables, name, offsets=sr.SHIFTED_MAPS)
        assert shifted.bufs[2].ptr % 16 == 4 and shifted.bufs[0].ptr % 16 == 0 and shifted.W % 16 == 0
        shifted.prepare()
        assert eng9.soil_words_state() == state
        shifted.run(3, 1 << sr.K1, "one table")
        assert eng9.last_kernel_name().startswith("cn_strip_kernel<1")
        shifted.run(3, 0x1ff, "all tables")
        shifted.run(3, 0x1ff, "all tables, 13-row strips", strip_rows=13)
        assert eng9.last_kernel_name().startswith("cn_strip_kernel<0")
    finally:
        eng9.sync()
        aligned.close()
        if shifted is not None:
            shifted.close()


@pytest.mark.parametrize("name", ["A-zig-zag", "G-2048"])
@pytest.mark.parametrize("reader", READERS)
def test_h_the_prepared_soil_is_a_snapshot(eng9, tables, reader, name):
    """Case H: coarse and ci are overwritten once prepare_tile has run; the reader, first of the tile, makes the
    bytes from what the context kept (a complex tile and a compact one)."""
    t = make_tile(eng9, tables, name)
    try:
        t.prepare()
        eng9.sync()
        eng9.memset(t.bufs[1].ptr, 0xEE, t.coarse.nbytes)
        eng9.memset(t.bufs[2].ptr, 0xEE, t.ci.nbytes)
        eng9.sync()
        run_reader(t, reader)
    finally:
        eng9.sync()
        t.close()


@pytest.mark.parametrize("reader", READERS)
def test_i_tile_after_tile_on_one_context(eng9, tables, reader):
    """Case I: tile 1 with every reader run, so that its bytes are in the workspace; then a smaller tile, whose
    parts lie elsewhere in the same workspace, and a third as large as the first with other soil.  On tiles 2 and 3 the
    named reader is the first call after prepare_tile and must see that tile's soil, not what the workspace holds."""
    tiles = []
    try:
        for spec in sr.CASE_I:
            tiles.append(sr.ReaderTile(eng9, tables, key="I-%d" % spec["seed"], **spec))
        soils = sr.case_i_soils()
        for t, soil in zip(tiles, soils):
            np.testing.assert_array_equal(t.soil, soil)
        for a, b in ((0, 1), (1, 2), (0, 2)):       # on the inputs: were the soils alike, stale bytes would pass
            w = min(tiles[a].W, tiles[b].W)
            differ = sr.soil_code(soils[a][:, :w]) != sr.soil_code(soils[b][:, :w])
            assert differ.mean() > 0.5, (a, b)
        tiles[0].prepare()
        for every in READERS:
            run_reader(tiles[0], every)
        for t in tiles[1:]:
            t.prepare()
            run_reader(t, reader)
    finally:
        eng9.sync()
        for t in tiles:
            t.close()


DELAY_BYTES = 256 << 20


@pytest.fixture(scope="module")
def delay(engine):
    """Two buffers for a copy that keeps stream 1 busy (about 0.2 ms) while the second reader is launched."""
    bufs = [engine.alloc(DELAY_BYTES), engine.alloc(DELAY_BYTES)]
    yield bufs
    for b in bufs:
        b.close()


@pytest.mark.parametrize("W", [2048, 2051])
@pytest.mark.parametrize("second", READERS)
@pytest.mark.parametrize("first", READERS)
def test_two_readers_on_two_streams(eng9, tables, delay, first, second, W):
    """prepare_tile on the main stream, an event, and two side streams that wait for it: `first` runs on stream 1,
    `second` on stream 2, nothing else orders them, and both results are checked.  W = 2048: `first` makes the bytes
    and `second` waits on the context's event for them; W = 2051: prepare_tile made them and both wait.

    Truly concurrent -- both launches are queued before either is awaited -- are the pairs whose FIRST reader is
    strip, verify, histogram, zonal, overview, aggregate or grid (cn_strip, verify_strip, pair_histogram,
    zonal_pair_histogram_device, overview_average, aggregate and grid_sums / grid_sums_storms return at once); with
    fused second, its kernels are queued behind the event while the first reader may still run.  Only ordered are the
    eight pairs whose first reader is fused: deflate_fused downloads its streams and frees its arena, so stream 1 is
    idle when `second` is launched -- those pairs show that a reader on another stream finds the bytes, not that it waits for them.

    Stream 1 first copies 256 MiB, so that `second` is queued on an idle stream 2 before `first` has made the
    bytes, and every pair has soil of its own, so that the bytes the test before left behind are wrong ones."""
    seed = 1000 + (READERS.index(first) * len(READERS) + READERS.index(second)) * 2 + W % 2
    t = sr.ReaderTile(eng9, tables, seed, W, 40, 90, 6)
    s1 = s2 = ev = None
    rd = []
    try:
        s1, s2, ev = eng9.stream_create(), eng9.stream_create(), eng9.event_create()
        rd = [sr.READER_CLASSES[first](t), sr.READER_CLASSES[second](t)]
        t.prepare()
        eng9.event_record(ev)
        eng9.stream_wait_event(s1, ev)
        eng9.stream_wait_event(s2, ev)
        eng9.stream_copy(delay[0].ptr, delay[1].ptr, DELAY_BYTES, s1)
        rd[0].launch(s1)
        rd[1].launch(s2)
        eng9.sync(s1)
        eng9.sync(s2)
        rd[0].check()
        rd[1].check()
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
