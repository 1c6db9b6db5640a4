"""GPU: the sums on a model grid with k weight tables per cell, counted once (gcn10_gpu_grid_sums_rains,
gcn10_gpu_grid_finish_rains) through the ABI face.  Needs an MI355X.

Inputs and shapes: those of tests/test_gpu_grid_rain.py (its strip of 1043 x 61, field_for's recipe per layer, map_of,
the 256 TABLES), so that the oracle's rasters of a strip are computed once for both files.  Expected values
(tests/rainsutil.py): words 0 and 1 from gridutil, word 2 + j from rainutil.add_triples with field j, the bytes from
rainutil.cn_cells with field j; equality with the _rain pair of calls at k = 1 is a cross-check beside that.  Every
comparison is bit for bit, and poison guards stand around acc, cnq and shared.  Every strip here stays at the launch's
floor of 16 rows per item; taller items are run in tests/test_gpu_rains_tall_items.py.
"""
import numpy as np
import pytest

from gcn10_amd import gpu
from tests import rainsutil as rs
from tests import stormutil
from tests.test_gpu_aggregate import Inputs, inputs, scene  # noqa: F401  (the recipe, its cache and the fixture)
from tests.test_gpu_grid import maps
from tests.test_gpu_grid_rain import Q50, ROWS1, TABLES, W1, map_of, run_finish_rain, run_rain, strip
from tests.test_runoff_host import hand_made_triples

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_STATE = 0, -1, -4
INT_MIN = -2 ** 31
POISON = rs.POISON

CELLS_1043 = {
    "8 x 8, the floor": lambda: maps(W1, ROWS1, 8, 8, (5, 3), (3, 2)),
    "25 and 26 in turn": lambda: (map_of(W1, (25, 26), 5, 3), map_of(ROWS1, (25, 26), 3, 2)),
    "120 x 50": lambda: maps(W1, ROWS1, 120, 50, (5, 3), (3, 2)),
    "one cell over everything": lambda: maps(W1, ROWS1, 1e6, 1e6, (5, 3), (3, 2)),
}


def shape_of(cellx, celly):
    return int(cellx.max()) + 1, int(celly.max()) + 1


# ---- random, different fields against the restatement ---------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 3, 8])
@pytest.mark.parametrize("cells", sorted(CELLS_1043))
def test_random_fields_equal_the_summed_oracle(scene, tables, cells, k):
    """-1 columns and rows on all four sides, the landcover at an odd byte offset; both conditions, then one condition
    and one raster."""
    sc = strip(scene, tables)
    assert sc.esa_ptr % 2 == 1
    cellx, celly = CELLS_1043[cells]()
    ncx, ncy = shape_of(cellx, celly)
    fields = rs.fields_for(k, ncx, ncy)
    got = rs.check_rains(sc, cellx, celly, fields, TABLES)
    assert got.shape == (18, ncy, ncx, 2 + k) and got[..., 1].max() > 0 and (got[..., 2:].max(axis=(0, 1, 2)) > 0).all()
    rs.check_rains(sc, cellx, celly, fields, TABLES, cond_mask=2)
    rs.check_rains(sc, cellx, celly, fields, TABLES, cond_mask=1, table_mask=1 << 4)


def test_k_1_gives_the_words_and_bytes_of_the_rain_pair(scene, tables):
    """Beside the restatement: the two pairs of calls write the same words and the same bytes."""
    sc = strip(scene, tables)
    cellx, celly = (map_of(W1, (25, 26), 5, 3), map_of(ROWS1, (25, 26), 3, 2))
    ncx, ncy = shape_of(cellx, celly)
    fields = rs.fields_for(1, ncx, ncy)
    fields[0, 0, :4] = (0, 3, 7, 255)       # no rain, a table that decreases, and the largest depth
    got = rs.check_rains(sc, cellx, celly, fields, TABLES)
    np.testing.assert_array_equal(got, run_rain(sc, cellx, celly, fields[0], TABLES))
    flat = got.reshape(18, -1, 3)
    idx = [0, ncx * ncy - 1, 7, 7]
    means, cnq, shared = rs.run_finish_rains(sc.eng, flat, fields, TABLES, idx)
    r_means, r_cnq, r_shared = run_finish_rain(sc.eng, flat, fields[0], TABLES, idx)
    np.testing.assert_array_equal(means, r_means)
    np.testing.assert_array_equal(cnq[0], r_cnq)
    np.testing.assert_array_equal(shared, r_shared)
    w_means, w_cnq = rs.want_bytes(flat, fields, TABLES)
    np.testing.assert_array_equal(means, w_means)
    np.testing.assert_array_equal(cnq, w_cnq)


def test_entries_that_name_no_table_count_as_table_0(scene, tables):
    sc = strip(scene, tables)
    cellx, celly = maps(W1, ROWS1, 25, 25.6, (5, 3), (3, 2))
    ncx, ncy = shape_of(cellx, celly)
    fields = rs.fields_for(2, ncx, ncy)
    seven = TABLES[:7]
    assert (fields[1] >= 7).any() and (fields[1] < 7).any()
    got = rs.check_rains(sc, cellx, celly, fields, seven)
    zero = fields.copy()
    zero[zero >= 7] = 0
    np.testing.assert_array_equal(got, rs.run_rains(sc, cellx, celly, zero, seven))


def test_a_dry_layer_and_two_equal_layers(scene, tables):
    """Layer 1 of four is all 0: its word is 0 everywhere and its bytes are the mean bytes.  Layers 0 and 3 are equal:
    equal words and bytes."""
    sc = strip(scene, tables)
    assert not TABLES[0].any()
    cellx, celly = maps(W1, ROWS1, 25, 25.6, (5, 3), (3, 2))
    ncx, ncy = shape_of(cellx, celly)
    fields = rs.fields_for(4, ncx, ncy)
    fields[1] = 0
    fields[3] = fields[0]
    got = rs.check_rains(sc, cellx, celly, fields, TABLES)
    assert (got[..., 3] == 0).all() and got[..., 2].max() > 0
    np.testing.assert_array_equal(got[..., 5], got[..., 2])
    assert (got[..., 4] != got[..., 2]).any()
    flat = got.reshape(18, -1, 6)
    means, cnq, _ = rs.run_finish_rains(sc.eng, flat, fields, TABLES, [])
    w_means, w_cnq = rs.want_bytes(flat, fields, TABLES)
    np.testing.assert_array_equal(means, w_means)
    np.testing.assert_array_equal(cnq, w_cnq)
    np.testing.assert_array_equal(cnq[1], means)
    np.testing.assert_array_equal(cnq[3], cnq[0])


# ---- items and pieces -----------------------------------------------------------------------------------------------

def test_one_cell_over_several_items_each_way_beside_narrow_ones(scene, tables):
    """The 4099 x 300 strip of tests/test_gpu_grid_rain.py: a cell that at least three items each way add to, k = 3."""
    cols, rows = gpu.grid_rain_item()
    W, H = 4099, 300
    wide, tall = 2 * cols + 40, 2 * rows + 10
    assert 1000 + wide + 100 <= W and 20 + tall + 8 <= H, "the strip no longer holds three items each way"
    sc = scene(inputs(("rain tall", W), W, H, 25, 19, tables))
    narrow_x = (1000 - 5) // 25
    cellx = map_of(W, [25] * narrow_x + [wide] + [25] * 1000, 5, 3)
    celly = map_of(H, [20, tall, 8, 8, 8, 8], 0, 2)
    big_x, big_y = narrow_x, 1
    x = np.flatnonzero(cellx == big_x)
    y = np.flatnonzero(celly == big_y)
    assert len(x) == wide and len(y) == tall and x[-1] // cols - x[0] // cols >= 2
    ncx, ncy = shape_of(cellx, celly)
    got = rs.check_rains(sc, cellx, celly, rs.fields_for(3, ncx, ncy), TABLES, table_mask=0x81)
    assert got[0, big_y, big_x, 1] > 0 and (got[0, big_y, big_x, 2:] > 0).all()


def test_one_single_pair_with_cell_edges_inside_a_wave_a_lane_and_on_a_group_boundary(scene, tables):
    """Constant landcover and soil, so that whole waves take the one-add path of count16; cell edges 16 k + 7 and 16 k,
    k = 2."""
    W, H = 2100, 24
    inp = Inputs(W, H, 25, 77, tables)
    inp.esa[:] = 40
    inp.coarse[:] = 2
    inp.soil = inp.coarse[inp.cj[:, None], inp.ci[None, :]]
    sc = scene(inp)
    cellx = np.full(W, -1, np.int32)
    for k, (a, b) in enumerate(((0, 80), (80, 151), (151, 1207), (1207, 1216), (1216, 2100))):
        cellx[a:b] = k
    celly = map_of(H, (9, 15), 0, 0)
    got = rs.check_rains(sc, cellx, celly, rs.fields_for(2, 5, 2), TABLES)
    np.testing.assert_array_equal(got[0, :, :, 1], np.outer([9, 15], [80, 71, 1056, 9, 884]))


def test_a_piece_of_more_than_64_bins(scene, tables):
    """Landcover drawn from all 256 bytes, pixel by pixel: a cell of 120 x 50 pixels holds more than 64 distinct
    landcover bytes, so more than 64 non-zero bins, and a lane meets several -- its first in registers, the others in
    LDS again for every word.  k = 8."""
    inp = Inputs(W1, ROWS1, 25, 31, tables)
    inp.esa = np.random.default_rng(32).integers(0, 256, inp.esa.shape).astype(np.uint8)
    sc = scene(inp)
    cellx, celly = maps(W1, ROWS1, 120, 50, (5, 3), (3, 2))
    ncx, ncy = shape_of(cellx, celly)
    for cy in range(ncy):
        for cx in range(ncx):
            piece = inp.esa[np.ix_(celly == cy, cellx == cx)]
            # a bin is a (landcover byte, soil class) pair: at least as many as there are landcover bytes
            assert len(np.unique(piece)) > 64 or piece.size < 1000, (cy, cx, len(np.unique(piece)))
    piece = inp.esa[np.ix_(celly == 0, cellx == 0)]
    assert len(np.unique(piece)) > 192                      # three bins and more for some lanes
    got = rs.check_rains(sc, cellx, celly, rs.fields_for(8, ncx, ncy), TABLES)
    assert (got[..., 2:].max(axis=(0, 1, 2)) > 0).all()
    rs.check_rains(sc, cellx, celly, rs.fields_for(8, ncx, ncy), TABLES, cond_mask=2, table_mask=0x41)
    # and one cell over everything: every bin of the strip in one piece
    cellx, celly = maps(W1, ROWS1, 1e6, 1e6, (5, 3), (3, 2))
    rs.check_rains(sc, cellx, celly, rs.fields_for(8, 1, 1, seed=9), TABLES)


def test_sums_beyond_32_bits(scene):
    """A cell of 90 601 pixels of value 100 with the table "all 65535" in layer 1 of 2: that word passes 2^32."""
    t = np.full((9, 256, 5), 100, np.int32)
    W = H = 301
    inp = Inputs(W, H, 25, 5, t)
    inp.coarse[:] = 2                       # a valid soil everywhere: no pixel is 255
    inp.soil = inp.coarse[inp.cj[:, None], inp.ci[None, :]]
    sc = scene(inp)
    cellx, celly = np.zeros(W, np.int32), np.zeros(H, np.int32)
    w = np.stack([Q50, stormutil.POOL["all 65535"]])
    fields = np.array([0, 1], np.uint8).reshape(2, 1, 1)
    got = rs.check_rains(sc, cellx, celly, fields, w, table_mask=0x11)
    n = got[0, 0, 0, 1]
    assert n >= 90000 and got[0, 0, 0, 0] == 100 * n and got[0, 0, 0, 3] == 65535 * n > (1 << 32)
    assert got[0, 0, 0, 2] == int(Q50[100]) * n


# ---- ADD semantics --------------------------------------------------------------------------------------------------

def test_two_calls_cut_inside_a_cell_row_add_up_to_one_and_a_second_call_doubles(scene, tables):
    sc = strip(scene, tables)
    cellx, celly = maps(W1, ROWS1, 100, 25.6, (5, 3), (3, 2))
    fields = rs.fields_for(3, *shape_of(cellx, celly))
    whole = rs.check_rains(sc, cellx, celly, fields, TABLES)
    cut = 31
    assert celly[cut - 1] == celly[cut] >= 0
    parts = rs.run_rains(sc, cellx, celly, fields, TABLES, bands=[(0, cut), (cut, ROWS1 - cut)])
    np.testing.assert_array_equal(parts, whole)
    twice = rs.run_rains(sc, cellx, celly, fields, TABLES, repeat=2)
    np.testing.assert_array_equal(twice, 2 * whole)
    assert whole[..., 1].max() > 0 and whole[..., 2:].max() > 0


# ---- memory safety --------------------------------------------------------------------------------------------------

def test_maps_and_fields_that_break_the_rules_write_nothing_outside(scene, tables):
    """Map entries >= ncx, >= ncy, negative and INT_MIN count as "in no cell", field entries >= the table count as table
    0; the guards around acc stay (run_rains asserts it), cell_tables has exactly k * ncy * ncx bytes, and the words are
    those of the valid entries.  Then the maps reversed: entries that decrease are summed all the same."""
    sc = strip(scene, tables)
    cellx, celly = maps(W1, ROWS1, 8, 8, (5, 3), (3, 2))
    ncx, ncy = int(cellx.max()) + 1 - 3, int(celly.max()) + 1 - 1      # the last cells are beyond acc
    rng = np.random.default_rng(8)
    cellx, celly = cellx.copy(), celly.copy()
    for m, n in ((cellx, ncx), (celly, ncy)):
        at = rng.permutation(len(m))[:len(m) // 6]
        m[at] = rng.choice([INT_MIN, -7, n, n + 5, 2 ** 31 - 1, -1], len(at))
    fields = rs.fields_for(3, ncx, ncy)
    assert (fields >= 7).any() and (cellx >= ncx).any() and (celly >= ncy).any() and (cellx == INT_MIN).any()
    rs.check_rains(sc, cellx, celly, fields, TABLES[:7])
    rs.check_rains(sc, cellx[::-1].copy(), celly[::-1].copy(), fields, TABLES[:7], table_mask=0x3)


# ---- grid_finish_rains ----------------------------------------------------------------------------------------------

def test_finish_on_hand_made_words(engine, tables):
    """hand_made_triples extended to 2 + 3 words: every branch of the cell rule against a rising table (bisection) and
    one that decreases (the scan), a field entry that names no table, n = 0, sw = 0 and words no c reaches; shared
    cells packed with n_shared > 0 and = 0."""
    engine.set_tables(tables)
    down = Q50.copy()
    down[40:60] = down[40:60][::-1]
    three = np.stack([Q50, down, stormutil.POOL["random"]])
    triples = hand_made_triples(Q50) + [(50, 1, 65536), (50 << 20, 1 << 20, 65535 << 21), (7, 1, 1 << 40)]
    n = len(triples)
    # layer 0 carries the hand-made sw, layer 1 the sw of the triple behind it, layer 2 half of it
    words = [(s, c, sw, triples[(i + 1) % n][2], sw // 2) for i, (s, c, sw) in enumerate(triples)]
    acc = np.array([words, words[::-1]], np.int64)
    fields = np.stack([(np.arange(n) % 5), (np.arange(n) + 1) % 3, np.full(n, 1)]).astype(np.uint8)
    assert (fields[0] >= 3).any()                           # 3 and 4 name no table: table 0
    idx = [0, n - 1, 3, 3, 0]
    means, cnq, shared = rs.run_finish_rains(engine, acc, fields, three, idx)
    w_means, w_cnq = rs.want_bytes(acc, fields, three)
    np.testing.assert_array_equal(means, w_means)
    np.testing.assert_array_equal(cnq, w_cnq)
    np.testing.assert_array_equal(shared, acc[:, idx, :])
    assert (cnq[0][0][:2] == 255).all() and 100 in cnq[0][0][-3:]
    assert (cnq[2] != cnq[0]).any() and (cnq[1] != cnq[0]).any()
    means, cnq, shared = rs.run_finish_rains(engine, acc, fields, three, [])    # n_shared = 0: no pointer is touched
    np.testing.assert_array_equal(cnq, w_cnq)
    assert shared.shape == (2, 0, 5)


# ---- state and errors -----------------------------------------------------------------------------------------------

def _sums(eng, esa, cj, cx, cy, field, acc, W=32, rows=4, ncx=2, ncy=1, cond=3, table=0x1FF, k=2):
    rc = gpu.lib().gcn10_gpu_grid_sums_rains(eng._ctx, esa, W, rows, cj, cx, cy, ncx, ncy, cond, table, field, k, acc,
                                             None)
    return rc, gpu.lib().gcn10_gpu_last_error().decode()


def test_state_and_errors(tables):
    eng = gpu.Engine(0)
    L = gpu.lib()
    try:
        inp = Inputs(32, 4, 8, 3, tables)
        cellx, celly = (np.arange(32) // 16).astype(np.int32), np.zeros(4, np.int32)
        fields = np.array([[1, 9], [0, 1]], np.uint8)       # 9 names no table: table 0
        bufs = [eng.upload(a) for a in (inp.esa, inp.coarse, inp.ci, inp.cj, cellx, celly, fields)]
        nbytes = 18 * 2 * 8 * 4
        acc = eng.alloc(nbytes)
        out = eng.alloc(256)
        eng.memset(acc.ptr, POISON, nbytes)
        eng.memset(out.ptr, POISON, 256)
        esa, cj, cx, cy, fld = bufs[0].ptr, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr, bufs[6].ptr
        o = out.ptr
        two = np.ascontiguousarray(np.stack([stormutil.POOL["random"], Q50]))
        rc, msg = _sums(eng, esa, cj, cx, cy, fld, acc.ptr)
        assert rc == E_STATE and "gcn10_gpu_set_tables" in msg, (rc, msg)
        eng.set_tables(tables)
        eng.prepare_tile(bufs[1].ptr, inp.hsx, inp.hsy, bufs[2].ptr, 32)
        rc, msg = _sums(eng, esa, cj, cx, cy, fld, acc.ptr)
        assert rc == E_STATE and "gcn10_gpu_set_rain_tables" in msg, (rc, msg)
        rc = L.gcn10_gpu_grid_finish_rains(eng._ctx, acc.ptr, 18, 2, fld, 2, o, o + 64, None, 0, None, None)
        assert rc == E_STATE and "gcn10_gpu_set_rain_tables" in L.gcn10_gpu_last_error().decode()
        eng.set_rain_tables(two)
        eng.set_tables(tables)              # does not void the rain tables
        rc, msg = _sums(eng, esa, cj, cx, cy, fld, acc.ptr, W=48)
        assert rc == E_STATE and "prepare" in msg, (rc, msg)
        bad = [dict(k=0), dict(k=9), dict(k=-1), dict(rows=0), dict(rows=-1), dict(ncx=0), dict(ncx=-2), dict(ncy=0),
               dict(ncy=-1), dict(cond=0), dict(cond=4), dict(table=0), dict(table=1 << 9), dict(cx=None), dict(cy=None),
               dict(field=None), dict(acc=None)]
        for kw in bad:
            args = dict(cx=cx, cy=cy, field=fld, acc=acc.ptr)
            args.update(kw)
            rc, msg = _sums(eng, esa, cj, **args)
            assert rc == E_INVAL and "gcn10_gpu_grid_sums_rains" in msg, (kw, rc, msg)
        for args in ((acc.ptr, 0, 2, fld, 2, o, o + 64, None, 0, None), (acc.ptr, 19, 2, fld, 2, o, o + 64, None, 0, None),
                     (acc.ptr, 18, 0, fld, 2, o, o + 64, None, 0, None), (None, 18, 2, fld, 2, o, o + 64, None, 0, None),
                     (acc.ptr, 18, 2, None, 2, o, o + 64, None, 0, None), (acc.ptr, 18, 2, fld, 0, o, o + 64, None, 0, None),
                     (acc.ptr, 18, 2, fld, 9, o, o + 64, None, 0, None), (acc.ptr, 18, 2, fld, -1, o, o + 64, None, 0, None),
                     (acc.ptr, 18, 2, fld, 2, None, o + 64, None, 0, None), (acc.ptr, 18, 2, fld, 2, o, None, None, 0, None),
                     (acc.ptr, 18, 2, fld, 2, o, o + 64, None, 1, acc.ptr), (acc.ptr, 18, 2, fld, 2, o, o + 64, cx, 1, None)):
            rc = L.gcn10_gpu_grid_finish_rains(eng._ctx, *args, None)
            assert rc == E_INVAL and "gcn10_gpu_grid_finish_rains" in L.gcn10_gpu_last_error().decode(), args
        eng.sync()
        assert (eng.download(acc.ptr, (nbytes,)) == POISON).all(), "a refused call wrote"
        assert (eng.download(out.ptr, (256,)) == POISON).all(), "a refused call wrote"
        # and the good call, after all that
        eng.memset(acc.ptr, 0, nbytes)
        rc, msg = _sums(eng, esa, cj, cx, cy, fld, acc.ptr)
        assert rc == OK, msg
        eng.sync()
        got = eng.download(acc.ptr, (nbytes,)).view(np.uint64).astype(np.int64).reshape(18, 1, 2, 4)
        rs.same_words(got, rs.want_words(inp, cellx, celly, fields.reshape(2, 1, 2), two), "the good call")
    finally:
        eng.sync()
        eng.close()
