"""GPU: several weight tables in one pass on a model grid (gcn10_gpu_set_weight_tables, gcn10_gpu_grid_sums_storms,
gcn10_gpu_grid_finish_storms) through the ABI face.  Needs an MI355X.

Inputs: the recipe of tests/test_gpu_aggregate.py, the maps, the guards and the poison of tests/test_gpu_grid.py.
Expected values: the oracle's full-resolution rasters, accumulated in numpy int64 over the maps with one more word per
table (tests/stormutil.py::add_words, held to runoffutil.add_triples by tests/test_storms_host.py), and the cell rule in
numpy per table (runoffutil.cn_array).  Every comparison is bit-exact.  The sets of tables are turns of one ring of the
adversarial tables of tests/test_gpu_grid_runoff.py -- every low byte 255, every high byte 255, all 65535, random -- and
the real tables of 25 / 50 / 100 mm, so that every slot j of 0..7 gets an adversarial table in some case: a plane added
to the wrong word, or with the wrong shift, shows.
"""
import numpy as np
import pytest

from gcn10_amd import gpu, host
from tests import aggutil as au
from tests import gridutil as gu
from tests import runoffutil as ru
from tests import stormutil as su
from tests.test_gpu_aggregate import Inputs, Scene, inputs, scene  # noqa: F401  (the recipe, its cache and the fixture)
from tests.test_gpu_capped_grids import band_rows, cus, finish_shape, triple_pool  # noqa: F401  (shape rules, fixture)
from tests.test_gpu_grid import GUARD, POISON, ROWS, WORKGROUP_PX, maps, run_finish, run_sums, want_sums
from tests.test_gpu_grid_runoff import Q50, run_weighted
from tests.test_runoff_host import hand_made_triples

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_STATE = 0, -1, -4
WIDTHS = [17, 1041, 4200, 36001]            # 36001: nine chunks, a last group of one pixel
CELLS = [(8, 8), (25, 25.6), (1e6, 16)]     # (8, 8): three masks per lane
# the launch arithmetic of gcn10_grid.hip (launch_sums): bands of at least 16 rows, chunks of 4096 columns, items dealt
# in groups of eight
BAND_FLOOR, CHUNK = 16, 4096


def case_of(W, i):
    """(k, turn of the ring, table_mask) of width W with cell size i: every k at every width but one, and at the block
    width four rasters only (18 x 8 expected words of two million pixels take too long)"""
    wi = WIDTHS.index(W)
    return su.KS[(wi + i) % 4], 2 * wi + 3 * i, 0x81 if W == 36001 else 0x1FF


def items_of(W, rows):
    """work items of a call while the bands stay at their floor of 16 rows"""
    return -(-W // CHUNK) * -(-rows // BAND_FLOOR)


def run_storms(sc, cellx, celly, ws, cond_mask=3, table_mask=0x1FF, bands=None, repeat=1):
    """int64[n_sel][ncy][ncx][2 + k] after set_weight_tables(ws) and grid_sums_storms over the scene's strip -- in one
    call, or one call per (y0, rows) of `bands` --, `repeat` times; asserts that not a byte around the words was
    written."""
    inp, eng = sc.inp, sc.eng
    sel = au.selected(cond_mask, table_mask)
    words = 2 + len(ws)
    ncx, ncy = int(cellx.max()) + 1, int(celly.max()) + 1
    nbytes = len(sel) * ncy * ncx * 8 * words
    buf = eng.alloc(nbytes + 2 * GUARD)
    ups = [eng.upload(cellx), eng.upload(celly)]
    try:
        eng.set_weight_tables(ws)
        eng.memset(buf.ptr, POISON, nbytes + 2 * GUARD)
        eng.memset(buf.ptr + GUARD, 0, nbytes)
        for _rep in range(repeat):
            for y0, n in bands or [(0, len(celly))]:
                eng.grid_sums_storms(sc.esa_ptr + y0 * inp.W, inp.W, n, sc.bufs[3].ptr + 4 * y0, ups[0].ptr,
                                     ups[1].ptr + 4 * y0, ncx, ncy, cond_mask, table_mask, buf.ptr + GUARD)
        eng.sync()
        img = eng.download(buf.ptr, (nbytes + 2 * GUARD,))
    finally:
        eng.sync()
        for b in [buf] + ups:
            b.close()
    assert (img[:GUARD] == POISON).all() and (img[GUARD + nbytes:] == POISON).all(), "bytes around acc were written"
    return img[GUARD:GUARD + nbytes].view(np.uint64).astype(np.int64).reshape(len(sel), ncy, ncx, words)


def want_words(inp, cellx, celly, ws, cond_mask=3, table_mask=0x1FF):
    sel = au.selected(cond_mask, table_mask)
    acc = np.zeros((len(sel), int(celly.max()) + 1, int(cellx.max()) + 1, 2 + len(ws)), np.int64)
    for q, r in enumerate(sel):
        su.add_words(acc[q], inp.want(r)[:len(celly)], cellx, celly, ws)
    return acc


def check_storms(sc, cellx, celly, ws, cond_mask=3, table_mask=0x1FF, **kw):
    got = run_storms(sc, cellx, celly, ws, cond_mask, table_mask, **kw)
    want = want_words(sc.inp, cellx, celly, ws, cond_mask, table_mask)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "W=%d k=%d: %d of %d words differ, first (q, cy, cx, word) = %s: got %d, want %d" % (
        sc.inp.W, len(ws), len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    return got


def run_finish_storms(eng, acc, shared_idx, ws):
    """(means uint8[n_sel][n_cells], cnq uint8[k][n_sel][n_cells], shared int64[n_sel][n_shared][2 + k]) of
    set_weight_tables(ws) and grid_finish_storms over int64 words [n_sel][n_cells][2 + k]; asserts that not a byte
    around the three was written."""
    n_sel, n_cells, words = acc.shape
    k = words - 2
    assert k == len(ws)
    idx = np.asarray(shared_idx, np.uint32)
    n_sh, nb = len(idx), n_sel * n_cells
    d_acc = eng.upload(acc.astype(np.uint64))
    d_idx = eng.upload(idx) if n_sh else None
    out = [eng.alloc(nb + 2 * GUARD), eng.alloc(k * nb + 2 * GUARD), eng.alloc(n_sel * n_sh * 8 * words + 2 * GUARD)]
    try:
        eng.set_weight_tables(ws)
        for b in out:
            eng.memset(b.ptr, POISON, b.nbytes)
        eng.grid_finish_storms(d_acc.ptr, n_sel, n_cells, out[0].ptr + GUARD, out[1].ptr + GUARD,
                               d_idx.ptr if n_sh else None, n_sh, out[2].ptr + GUARD if n_sh else None)
        eng.sync()
        img = [eng.download(b.ptr, (b.nbytes,)) for b in out]
    finally:
        eng.sync()
        for b in [d_acc, d_idx] + out:
            if b is not None:
                b.close()
    for name, im in zip(("means", "cnq", "shared"), img):
        assert (im[:GUARD] == POISON).all() and (im[-GUARD:] == POISON).all(), "bytes around %s were written" % name
    return (img[0][GUARD:-GUARD].reshape(n_sel, n_cells), img[1][GUARD:-GUARD].reshape(k, n_sel, n_cells),
            img[2][GUARD:-GUARD].view(np.uint64).astype(np.int64).reshape(n_sel, n_sh, words))


# ---- 1. widths, cell sizes, numbers of tables ------------------------------------------------------------------------

@pytest.mark.parametrize("W", WIDTHS)
def test_every_width_and_cell_size_equals_the_summed_oracle(scene, tables, W):
    inp = inputs(("grid", W), W, ROWS, 25, 70 + W, tables)
    sc = scene(inp)                                         # landcover one byte into its allocation
    widest = 0
    for i, (wx, wy) in enumerate(CELLS):
        lead, trail = ((5, 3), (3, 2)) if W > 30 else ((0, 0), (0, 0))
        cellx, celly = maps(W, ROWS, wx, wy, lead, trail)
        k, turn, table_mask = case_of(W, i)
        ws = su.table_set(k, turn)
        got = check_storms(sc, cellx, celly, ws, 3, table_mask)
        assert got.shape[-1] == 2 + k
        # words 0 and 1 against the unweighted call on the same maps: a cross-check, not the parity claim
        np.testing.assert_array_equal(got[..., :2], run_sums(sc, cellx, celly, 3, table_mask))
        if k == 1:      # one table: the whole array is what the weighted call adds
            np.testing.assert_array_equal(got, run_weighted(sc, cellx, celly, ws[0], 3, table_mask))
        widest = max(widest, int(np.bincount(cellx[cellx >= 0]).max()))
    if W == 4200:
        assert widest > WORKGROUP_PX    # one cell summed by two workgroups' columns


def test_every_slot_meets_an_adversarial_table():
    """From the shapes alone: which k and which tables every (width, cell size) gets."""
    seen, ks = {}, set()
    for W in WIDTHS:
        ks_here = set()
        for i in range(len(CELLS)):
            k, turn, _mask = case_of(W, i)
            ks.add(k)
            ks_here.add(k)
            for j, name in enumerate(su.table_names(k, turn)):
                seen.setdefault(j, set()).add(name)
        assert len(ks_here) == 3
    assert ks == set(su.KS) and sorted(seen) == list(range(8))
    for j in range(8):
        assert seen[j] & set(su.ADVERSARIAL), (j, seen[j])
    assert {case_of(36001, i)[0] for i in range(3)} >= {8}              # and eight tables at the block width
    assert set(su.ADVERSARIAL) <= seen[0] and set(su.ADVERSARIAL) <= seen[1]


# ---- 2. dealing ------------------------------------------------------------------------------------------------------

def test_the_roles_of_every_item_are_dealt(scene, tables, cus):  # noqa: F811
    """Eight tables: 17 roles per condition.  Both conditions (34 roles), one (17), table-mask subsets that leave a
    condition's workgroups without a raster only through cond_mask; item counts of 1, 4 and 36 -- no multiple of eight:
    the last group of every launch is padded, at 36 items half of it."""
    ws = su.table_set(8, 1)
    for W, rows, n_items in ((17, 16, 1), (17, ROWS, 4), (1041, ROWS, 4), (36001, ROWS, 36)):
        assert items_of(W, rows) == n_items and n_items % 8 != 0
        for roles in (17, 34):                              # on this device the bands of these calls are at the floor
            assert band_rows(W, rows, roles, cus) == BAND_FLOOR
        inp = inputs(("grid", W), W, ROWS, 25, 70 + W, tables)
        sc = scene(inp)
        cellx, celly = maps(W, ROWS, 8, 8, (5, 3) if W > 30 else (0, 0), (3, 2) if W > 30 else (0, 0))
        celly = celly[:rows]
        for cond_mask, table_mask in ((3, 0x81), (1, 0x81), (2, 0x100)) if W == 36001 else \
                ((3, 0x1FF), (1, 0x1FF), (2, 0x015), (3, 0x100)):
            got = check_storms(sc, cellx, celly, ws, cond_mask, table_mask)
            assert got.shape[0] == len(au.selected(cond_mask, table_mask)) and got[..., 2:].max() > 0
    assert items_of(36001, ROWS) % 8 == 4                   # half of the last group of eight is padding


@pytest.mark.parametrize("n_tables", [9, 5])
def test_awkward_tables_and_mask_subsets(scene, n_tables):
    from tests.util import random_tables
    t = random_tables(5, n_tables)
    inp = inputs(("grid nasty", n_tables), 333, 77, 25, 41, t)
    sc = scene(inp)
    full = (1 << n_tables) - 1
    cellx, celly = maps(333, 77, 8.5, 8, (2, 1), (1, 2))
    turn = 0
    for cond_mask in (1, 2, 3):
        for table_mask in (full, 1, 1 << (n_tables - 1), 0x15 & full):     # all, one raster per condition, a subset
            k = su.KS[turn % 4]
            got = check_storms(sc, cellx, celly, su.table_set(k, turn), cond_mask, table_mask)
            assert got.shape[0] == len(au.selected(cond_mask, table_mask))
            turn += 1


# ---- 3. one cell beyond 32 bits --------------------------------------------------------------------------------------

def test_one_cell_beyond_32_bits(scene, tables):
    """One cell over more than the 4096 columns of a workgroup and more than the 256 rows of a band, two tables whose
    every weight is 65535: words 2 and 3 both pass 2^32, which a 32-bit word anywhere on the way would lose."""
    W, rows = 4200, 300
    inp = inputs(("grid runoff tall", W), W, rows, 25, 19, tables)
    sc = scene(inp)
    cellx, celly = maps(W, rows, 1e6, 1e6, (5, 3), (3, 2))
    assert cellx.max() == 0 and celly.max() == 0 and (cellx == 0).sum() > WORKGROUP_PX and (celly == 0).sum() > 256
    ws = np.stack([su.POOL["all 65535"]] * 2)
    got = check_storms(sc, cellx, celly, ws, table_mask=0x81)
    assert got.shape == (4, 1, 1, 4)
    for word in (2, 3):
        assert (got[..., word] > (1 << 32)).all() and (got[..., word] == 65535 * got[..., 1]).all()


# ---- 4. ADD semantics ------------------------------------------------------------------------------------------------

def test_two_bands_cut_inside_a_cell_row_add_up_to_one_call(scene, tables):
    inp = inputs(("grid", 1041), 1041, ROWS, 25, 70 + 1041, tables)
    sc = scene(inp)
    for (wx, wy), (k, turn) in (((8, 25), (3, 6)), ((100, 25.6), (8, 4))):
        cellx, celly = maps(1041, ROWS, wx, wy, (5, 3), (3, 2))
        ws = su.table_set(k, turn)
        whole = check_storms(sc, cellx, celly, ws)
        cut = 31
        assert celly[cut - 1] == celly[cut] >= 0                 # the cut lies inside a cell row
        parts = check_storms(sc, cellx, celly, ws, bands=[(0, cut), (cut, ROWS - cut)])
        np.testing.assert_array_equal(parts, whole)


def test_a_second_call_doubles_every_word(scene, tables):
    inp = inputs(("grid", 1041), 1041, ROWS, 25, 70 + 1041, tables)
    sc = scene(inp)
    cellx, celly = maps(1041, ROWS, 17.3, 15.9, (5, 3), (3, 2))
    ws = np.stack([su.POOL["25 mm"], su.POOL["50 mm"], su.POOL["100 mm"]])
    once = check_storms(sc, cellx, celly, ws)
    twice = run_storms(sc, cellx, celly, ws, repeat=2)
    np.testing.assert_array_equal(twice, 2 * once)
    assert once[..., 1].max() > 0 and (once[..., 2:].reshape(-1, 3).max(axis=0) > 0).all()


# ---- 5. grid_finish_storms -------------------------------------------------------------------------------------------

def _down(w):
    w = np.array(w, np.uint16)
    w[40:60] = w[40:60][::-1]
    assert (np.diff(w[1:101].astype(np.int64)) < 0).any()
    return w


def hand_made_words(ws):
    """int64[n][2 + k]: the hand-made triples of every table in turn, the table's sum in its own word and the sums
    that the other tables' triples hold at the same place in theirs"""
    lists = [hand_made_triples(w) for w in ws]
    out = []
    for own in range(len(ws)):
        for i, (s, cnt, _sw) in enumerate(lists[own]):
            # (a table whose threshold lies above 60 makes "n q[60] - 1" negative: no sum is, so 0 stands there)
            out.append([s, cnt] + [max(lists[j][i % len(lists[j])][2], 0) for j in range(len(ws))])
    return np.array(out, np.int64)


def test_finish_on_hand_made_sums(engine, tables):
    engine.set_tables(tables)
    # the middle table goes down somewhere: the scan for it, bisection for the two beside it
    ws = np.stack([su.POOL["25 mm"], _down(Q50), su.POOL["100 mm"]])
    cells = hand_made_words(ws)
    acc = np.array([cells, cells[::-1]], np.int64)
    want = [[ru.cn(c[0], c[1], c[2 + j], ws[j]) for c in cells.tolist()] for j in range(3)]
    assert want == [[host.runoff_cn(c[0], c[1], c[2 + j], ws[j]) for c in cells.tolist()] for j in range(3)]
    assert len({tuple(w) for w in want}) == 3
    for idx in ([0, len(cells) - 1, 3, 3, 0], []):          # repeated and unordered shared cells; none at all
        means, cnq, shared = run_finish_storms(engine, acc, idx, ws)
        for j in range(3):
            assert cnq[j][0].tolist() == want[j] and cnq[j][1].tolist() == want[j][::-1], j
        np.testing.assert_array_equal(means, gu.means(acc[..., :2]))
        np.testing.assert_array_equal(shared, acc[:, idx, :])
        assert shared.shape == (2, len(idx), 5)
    # one table: what grid_finish_weighted writes
    from tests.test_gpu_grid_runoff import run_finish_weighted
    one = acc[..., [0, 1, 3]]
    got = run_finish_storms(engine, one, [2, 0], ws[1:2])
    old = run_finish_weighted(engine, one, [2, 0], ws[1])
    np.testing.assert_array_equal(got[0], old[0])
    np.testing.assert_array_equal(got[1][0], old[1])
    np.testing.assert_array_equal(got[2], old[2])


def test_finish_on_the_sums_of_a_scene(scene, tables):
    inp = inputs(("grid", 1041), 1041, ROWS, 25, 70 + 1041, tables)
    sc = scene(inp)
    cellx, celly = maps(1041, ROWS, 8, 8, (5, 3), (3, 2))
    ws = np.stack([su.POOL["25 mm"], su.POOL["50 mm"], su.POOL["100 mm"]])
    acc = check_storms(sc, cellx, celly, ws)
    n = acc[..., 1]
    want = su.cn_arrays(acc, ws)
    # cells without a value, cells that shed nothing in the smallest storm only, cells that shed in all
    assert (n == 0).any() and ((n > 0) & (acc[..., 2] == 0) & (acc[..., 3] > 0)).any() and (acc[..., 2] > 0).any()
    flat = acc.reshape(18, -1, 5)
    n_cells = flat.shape[1]
    idx = [0, n_cells - 1, 7, 7, n_cells // 2]
    means, cnq, shared = run_finish_storms(sc.eng, flat, idx, ws)
    np.testing.assert_array_equal(means, gu.means(flat[..., :2]))
    np.testing.assert_array_equal(cnq, want.reshape(3, 18, -1))
    np.testing.assert_array_equal(shared, flat[:, idx, :])
    assert (cnq[:, n.reshape(18, -1) == 0] == 255).all()


# ---- 6. the finish pass beyond its grid cap --------------------------------------------------------------------------

def test_finish_strides_over_the_cells(engine, tables, cus):  # noqa: F811
    """The shape rule of tests/test_gpu_capped_grids.py: every lane finishes two elements, the first 257 three."""
    s = finish_shape(cus)
    engine.set_option("defaults", 0)                            # grid_blocks_per_cu = 16
    engine.set_tables(tables)
    ws = np.stack([Q50, _down(su.POOL["100 mm"])])
    rng = np.random.default_rng(23)
    pools = [triple_pool(w, seed=3 + j) for j, w in enumerate(ws)]
    m = min(len(p) for p in pools)
    pool = np.concatenate([pools[0][:m], pools[1][:m, 2:3]], axis=1)       # s, n, sw for table 0, sw for table 1
    pick = rng.integers(0, m, size=(s.n_sel, s.n_cells))
    pick[:, :min(m, s.n_cells)] = np.arange(min(m, s.n_cells))
    idx = rng.integers(0, s.n_cells, s.n_shared).astype(np.uint32)
    idx[:4] = (s.n_cells - 1, 0, 7, 7)
    acc = pool[pick]
    means, cnq, shared = run_finish_storms(engine, acc, idx, ws)
    want = su.cn_arrays(pool, ws)
    assert len(set(want[0].tolist())) > 50 and len(set(want[1].tolist())) > 50
    np.testing.assert_array_equal(means, gu.means(pool[:, :2])[pick])
    np.testing.assert_array_equal(cnq, want[:, pick])
    np.testing.assert_array_equal(shared, acc[:, idx, :])


# ---- 7. state and errors ---------------------------------------------------------------------------------------------

def _sums(L, name, eng, esa, cj, cx, cy, acc, W=32, rows=4, ncx=2, ncy=1, cond=3, table=0x1FF):
    rc = getattr(L, name)(eng._ctx, esa, W, rows, cj, cx, cy, ncx, ncy, cond, table, acc, None)
    return rc, L.gcn10_gpu_last_error().decode()


def test_state_and_errors(tables):
    eng = gpu.Engine(0)
    L = gpu.lib()
    try:
        inp = Inputs(32, 4, 8, 3, tables)
        cellx, celly = (np.arange(32) // 16).astype(np.int32), np.zeros(4, np.int32)
        bufs = [eng.upload(a) for a in (inp.esa, inp.coarse, inp.ci, inp.cj, cellx, celly)]
        ws = np.ascontiguousarray(np.stack([su.POOL["25 mm"], su.POOL["random"]]))
        nbytes = 18 * 2 * 8 * 4
        acc = eng.alloc(nbytes)
        out = eng.alloc(256)
        eng.memset(acc.ptr, POISON, nbytes)
        eng.memset(out.ptr, POISON, 256)
        esa, cj, cx, cy = bufs[0].ptr, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr
        finish = (acc.ptr, 18, 2, out.ptr, out.ptr + 64, None, 0, None)
        storms = "gcn10_gpu_grid_sums_storms"
        # tables of weights need the lookup tables; the calls need weights, and new ones after every set_tables
        rc = L.gcn10_gpu_set_weight_tables(eng._ctx, ws.ctypes.data, 2)
        assert rc == E_STATE and "gcn10_gpu_set_tables" in L.gcn10_gpu_last_error().decode()
        eng.set_tables(tables)
        eng.prepare_tile(bufs[1].ptr, inp.hsx, inp.hsy, bufs[2].ptr, 32)
        for _round in range(2):
            rc, msg = _sums(L, storms, eng, esa, cj, cx, cy, acc.ptr)
            assert rc == E_STATE and "gcn10_gpu_set_weight_tables" in msg, (rc, msg)
            rc = L.gcn10_gpu_grid_finish_storms(eng._ctx, *finish, None)
            assert rc == E_STATE and "gcn10_gpu_set_weight_tables" in L.gcn10_gpu_last_error().decode()
            for w, k in ((None, 2), (ws.ctypes.data, 0), (ws.ctypes.data, 9), (ws.ctypes.data, -1)):
                rc = L.gcn10_gpu_set_weight_tables(eng._ctx, w, k)
                assert rc == E_INVAL and "gcn10_gpu_set_weight_tables" in L.gcn10_gpu_last_error().decode(), (w, k)
            rc, msg = _sums(L, storms, eng, esa, cj, cx, cy, acc.ptr)
            assert rc == E_STATE, (rc, msg)                 # a refused set_weight_tables set nothing
            eng.set_weight_tables(ws)
            rc, msg = _sums(L, storms, eng, esa, cj, cx, cy, acc.ptr, W=48)
            assert rc == E_STATE and "prepare" in msg, (rc, msg)
            # two tables: the one-table calls name the calls to make instead
            rc, msg = _sums(L, "gcn10_gpu_grid_sums_weighted", eng, esa, cj, cx, cy, acc.ptr)
            assert rc == E_STATE and "gcn10_gpu_grid_sums_storms" in msg, (rc, msg)
            rc = L.gcn10_gpu_grid_finish_weighted(eng._ctx, *finish, None)
            assert rc == E_STATE and "gcn10_gpu_grid_finish_storms" in L.gcn10_gpu_last_error().decode()
            eng.set_tables(tables)                      # invalidates the weights (the prepared tile stays)
        eng.set_weight_tables(ws)
        bad = [dict(rows=0), dict(rows=-1), dict(ncx=0), dict(ncx=-2), dict(ncy=0), dict(ncy=-1), dict(cond=0),
               dict(cond=4), dict(table=0), dict(table=1 << 9), dict(cx=None), dict(cy=None), dict(acc=None)]
        for kw in bad:
            args = dict(cx=cx, cy=cy, acc=acc.ptr)
            args.update(kw)
            rc, msg = _sums(L, storms, eng, esa, cj, **args)
            assert rc == E_INVAL and storms in msg, (kw, rc, msg)
        o = out.ptr
        for args in ((acc.ptr, 0, 2, o, o + 64, None, 0, None), (acc.ptr, 19, 2, o, o + 64, None, 0, None),
                     (acc.ptr, 18, 0, o, o + 64, None, 0, None), (None, 18, 2, o, o + 64, None, 0, None),
                     (acc.ptr, 18, 2, None, o + 64, None, 0, None), (acc.ptr, 18, 2, o, None, None, 0, None),
                     (acc.ptr, 18, 2, o, o + 64, None, 1, acc.ptr), (acc.ptr, 18, 2, o, o + 64, cx, 1, None)):
            rc = L.gcn10_gpu_grid_finish_storms(eng._ctx, *args, None)
            assert rc == E_INVAL and "gcn10_gpu_grid_finish_storms" in L.gcn10_gpu_last_error().decode(), args
        eng.sync()
        assert (eng.download(acc.ptr, (nbytes,)) == POISON).all(), "a refused call wrote"
        assert (eng.download(out.ptr, (256,)) == POISON).all(), "a refused call wrote"
        # and the good calls, after all that; then one table through set_weights: the one-table calls work again
        eng.memset(acc.ptr, 0, nbytes)
        rc, msg = _sums(L, storms, eng, esa, cj, cx, cy, acc.ptr)
        assert rc == OK, msg
        eng.sync()
        got = eng.download(acc.ptr, (nbytes,)).view(np.uint64).astype(np.int64).reshape(18, 1, 2, 4)
        want = np.zeros((18, 1, 2, 4), np.int64)
        for r in range(18):
            su.add_words(want[r], au.oracle_rasters(inp.esa, inp.soil, tables, [r])[r], cellx, celly, ws)
        np.testing.assert_array_equal(got, want)
        eng.set_weights(ws[1])
        eng.memset(acc.ptr, 0, nbytes)
        rc, msg = _sums(L, "gcn10_gpu_grid_sums_weighted", eng, esa, cj, cx, cy, acc.ptr)
        assert rc == OK, msg
        eng.sync()
        got = eng.download(acc.ptr, (18 * 2 * 24,)).view(np.uint64).astype(np.int64).reshape(18, 1, 2, 3)
        np.testing.assert_array_equal(got, want[..., [0, 1, 3]])
    finally:
        eng.sync()
        eng.close()


# ---- 8. the plain calls on a context that holds tables ---------------------------------------------------------------

def test_the_plain_calls_take_no_table_from_the_context(tables):
    """One sums kernel and one finish kernel serve 0 to 8 tables through one launch each, and gcn10_gpu_grid_sums /
    gcn10_gpu_grid_finish are k = 0 whatever the context holds: on a context with eight tables set, slot 0 all 65535,
    they write the pairs, the means and the packed pairs of a fresh context on which no weights were ever set, and not
    a byte around them (run_sums and run_finish hold the guards; grid_finish is given no cnq).  A call that took the
    context's k would write 10 words per (raster, cell) and 8 bytes per cell more."""
    inp = inputs(("grid", 1041), 1041, ROWS, 25, 70 + 1041, tables)
    cellx, celly = maps(1041, ROWS, 8, 8, (5, 3), (3, 2))
    ws = su.table_set(8, su.ORDER.index("all 65535"))
    assert (ws[0] == 65535).all()
    rng = np.random.default_rng(31)
    n = rng.integers(1, 1 << 33, (2, 300))                  # sums beyond 32 bits, means of 0 .. 254
    pairs = np.stack([n * rng.integers(0, 255, (2, 300)) + rng.integers(0, 1 << 33, (2, 300)) % n, n], axis=-1)
    pairs[:, ::7, 1] = 0                                    # cells without a value
    pairs[:, 1::7, 0] = 5 * pairs[:, 1::7, 1] // 2          # exact halves, which round up, where n is even
    got = []
    for with_tables in (False, True):
        eng = gpu.Engine(0)
        try:
            sc = Scene(eng, inp)
            try:
                if with_tables:
                    eng.set_weight_tables(ws)
                got.append([run_sums(sc, cellx, celly)] + [run_finish(eng, pairs, idx) for idx in ([0, 299, 7, 7], [])])
            finally:
                sc.close()
        finally:
            eng.sync()
            eng.close()
    fresh, held = got
    np.testing.assert_array_equal(fresh[0], want_sums(inp, cellx, celly))
    np.testing.assert_array_equal(held[0], fresh[0])
    for (means, shared), (means0, shared0), idx in zip(held[1:], fresh[1:], ([0, 299, 7, 7], [])):
        np.testing.assert_array_equal(means0, gu.means(pairs))
        np.testing.assert_array_equal(shared0, pairs[:, idx, :])
        np.testing.assert_array_equal(means, means0)
        np.testing.assert_array_equal(shared, shared0)
