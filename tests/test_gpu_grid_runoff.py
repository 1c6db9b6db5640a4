"""GPU: the weighted sums on a model grid (gcn10_gpu_set_weights, gcn10_gpu_grid_sums_weighted,
gcn10_gpu_grid_finish_weighted) through the ABI face.  Needs an MI355X.

Inputs: the recipe of tests/test_gpu_aggregate.py and the maps of tests/test_gpu_grid.py.  Expected values: the oracle's
full-resolution rasters, accumulated in numpy int64 over the maps with one more word for w[v]
(tests/runoffutil.py::add_triples), and the cell rule in numpy (runoffutil.cn_array).  Every comparison is bit-exact.
The weight tables are chosen to break a plane-wise sum that is wrong: every low byte 255, every high byte 255, both (a
plane byte of 255 is a number, not "no value"), a random table, and the runoff table of a 50 mm storm.
"""
import numpy as np
import pytest

from gcn10_amd import gpu, host
from tests import aggutil as au
from tests import gridutil as gu
from tests import runoffutil as ru
from tests.test_gpu_aggregate import Inputs, inputs, scene  # noqa: F401  (the recipe, its cache and the fixture)
from tests.test_gpu_grid import GUARD, POISON, ROWS, WORKGROUP_PX, maps, run_sums
from tests.test_runoff_host import hand_made_triples
from tests.util import random_tables

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_STATE = 0, -1, -4
WIDTHS = [1, 15, 16, 17, 1041, 4200, 36001]        # 36001: nine chunks, a last group of one pixel
CELLS = [(8, 8), (25, 25.6), (17.3, 17.3), (1e6, 16)]
Q50 = ru.table(50, 0.2)
WEIGHTS = {
    "low bytes 255": np.full(256, 0x00FF, np.uint16),
    "high bytes 255": np.full(256, 0xFF00, np.uint16),
    "all 65535": np.full(256, 0xFFFF, np.uint16),
    "random": np.random.default_rng(5).integers(0, 65536, 256).astype(np.uint16),
    "50 mm": Q50,
}
NAMES = sorted(WEIGHTS)


def run_weighted(sc, cellx, celly, w, cond_mask=3, table_mask=0x1FF, bands=None, repeat=1):
    """int64[n_sel][ncy][ncx][3] after set_weights(w) and grid_sums_weighted over the scene's strip -- in one call, or
    one call per (y0, rows) of `bands` --, `repeat` times; asserts that not a byte around the triples was written."""
    inp, eng = sc.inp, sc.eng
    sel = au.selected(cond_mask, table_mask)
    ncx, ncy = int(cellx.max()) + 1, int(celly.max()) + 1
    nbytes = len(sel) * ncy * ncx * 24
    buf = eng.alloc(nbytes + 2 * GUARD)
    ups = [eng.upload(cellx), eng.upload(celly)]
    try:
        eng.set_weights(w)
        eng.memset(buf.ptr, POISON, nbytes + 2 * GUARD)
        eng.memset(buf.ptr + GUARD, 0, nbytes)
        for _rep in range(repeat):
            for y0, n in bands or [(0, len(celly))]:
                eng.grid_sums_weighted(sc.esa_ptr + y0 * inp.W, inp.W, n, sc.bufs[3].ptr + 4 * y0, ups[0].ptr,
                                       ups[1].ptr + 4 * y0, ncx, ncy, cond_mask, table_mask, buf.ptr + GUARD)
        eng.sync()
        img = eng.download(buf.ptr, (nbytes + 2 * GUARD,))
    finally:
        eng.sync()
        for b in [buf] + ups:
            b.close()
    assert (img[:GUARD] == POISON).all() and (img[GUARD + nbytes:] == POISON).all(), "bytes around acc were written"
    return img[GUARD:GUARD + nbytes].view(np.uint64).astype(np.int64).reshape(len(sel), ncy, ncx, 3)


def want_triples(inp, cellx, celly, w, cond_mask=3, table_mask=0x1FF):
    sel = au.selected(cond_mask, table_mask)
    acc = np.zeros((len(sel), int(celly.max()) + 1, int(cellx.max()) + 1, 3), np.int64)
    for q, r in enumerate(sel):
        ru.add_triples(acc[q], inp.want(r)[:len(celly)], cellx, celly, w)
    return acc


def check_weighted(sc, cellx, celly, w, cond_mask=3, table_mask=0x1FF, **kw):
    got = run_weighted(sc, cellx, celly, w, cond_mask, table_mask, **kw)
    want = want_triples(sc.inp, cellx, celly, w, cond_mask, table_mask)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "W=%d: %d of %d words differ, first (q, cy, cx, word) = %s: got %d, want %d" % (
        sc.inp.W, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    return got


def run_finish_weighted(eng, acc, shared_idx, w):
    """(means, cnq uint8[n_sel][n_cells], shared int64[n_sel][n_shared][3]) of set_weights(w) and grid_finish_weighted
    over int64 triples [n_sel][n_cells][3]; asserts that not a byte around the three was written."""
    n_sel, n_cells = acc.shape[:2]
    idx = np.asarray(shared_idx, np.uint32)
    n_sh, nb = len(idx), n_sel * n_cells
    d_acc = eng.upload(acc.astype(np.uint64))
    d_idx = eng.upload(idx) if n_sh else None
    out = [eng.alloc(nb + 2 * GUARD), eng.alloc(nb + 2 * GUARD), eng.alloc(n_sel * n_sh * 24 + 2 * GUARD)]
    try:
        eng.set_weights(w)
        for b in out:
            eng.memset(b.ptr, POISON, b.nbytes)
        eng.grid_finish_weighted(d_acc.ptr, n_sel, n_cells, out[0].ptr + GUARD, out[1].ptr + GUARD,
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
    return (img[0][GUARD:-GUARD].reshape(n_sel, n_cells), img[1][GUARD:-GUARD].reshape(n_sel, n_cells),
            img[2][GUARD:-GUARD].view(np.uint64).astype(np.int64).reshape(n_sel, n_sh, 3))


# ---- widths, cell sizes, weight tables ---------------------------------------------------------------------------

@pytest.mark.parametrize("W", WIDTHS)
def test_every_width_and_cell_size_equals_the_summed_oracle(scene, tables, W):
    inp = inputs(("grid", W), W, ROWS, 25, 70 + W, tables)
    sc = scene(inp)                                         # landcover one byte into its allocation
    widest = 0
    for i, (wx, wy) in enumerate(CELLS):
        lead, trail = ((5, 3), (3, 2)) if W > 30 else ((0, 0), (0, 0))
        cellx, celly = maps(W, ROWS, wx, wy, lead, trail)
        # every weight table on the cells of 8 pixels of the 1041-column strip, one of them, in turn, elsewhere
        for name in NAMES if (W, i) == (1041, 0) else [NAMES[(i + W) % len(NAMES)]]:
            got = check_weighted(sc, cellx, celly, WEIGHTS[name])
        # words 0 and 1 against the unweighted call on the same maps: a cross-check, not the parity claim
        np.testing.assert_array_equal(got[..., :2], run_sums(sc, cellx, celly))
        widest = max(widest, int(np.bincount(cellx[cellx >= 0]).max()))
    if W == 4200:
        assert widest > WORKGROUP_PX    # one cell summed by two workgroups' columns


def test_the_wide_strips_meet_every_weight_table():
    """From the shapes alone: which table every (width, cell size) gets."""
    for W in (1041, 4200):
        used = {NAMES[(i + W) % len(NAMES)] for i in range(len(CELLS))}
        assert len(used) == 4
    assert {NAMES[(i + W) % len(NAMES)] for W in WIDTHS for i in range(len(CELLS))} == set(NAMES)


def test_one_cell_beyond_32_bits(scene, tables):
    """One cell over more than the 4096 columns of a workgroup and more than the 256 rows of a band, every weight 65535:
    the cell's third word passes 2^32, which a 32-bit word anywhere on the way would lose."""
    W, rows = 4200, 300
    inp = inputs(("grid runoff tall", W), W, rows, 25, 19, tables)
    sc = scene(inp)
    cellx, celly = maps(W, rows, 1e6, 1e6, (5, 3), (3, 2))
    assert cellx.max() == 0 and celly.max() == 0 and (cellx == 0).sum() > WORKGROUP_PX and (celly == 0).sum() > 256
    got = check_weighted(sc, cellx, celly, WEIGHTS["all 65535"], table_mask=0x81)
    assert got.shape == (4, 1, 1, 3)
    assert (got[..., 2] > (1 << 32)).all() and (got[..., 2] == 65535 * got[..., 1]).all()
    check_weighted(sc, cellx, celly, WEIGHTS["random"], table_mask=0x81)


@pytest.mark.parametrize("n_tables", [9, 5])
def test_awkward_tables_and_mask_subsets(scene, n_tables):
    t = random_tables(5, n_tables)
    inp = inputs(("grid nasty", n_tables), 333, 77, 25, 41, t)
    sc = scene(inp)
    full = (1 << n_tables) - 1
    cellx, celly = maps(333, 77, 8.5, 8, (2, 1), (1, 2))
    k = 0
    for cond_mask in (1, 2, 3):
        for table_mask in (full, 1, 1 << (n_tables - 1), 0x15 & full):     # all, one raster per condition, a subset
            got = check_weighted(sc, cellx, celly, WEIGHTS[NAMES[k % len(NAMES)]], cond_mask, table_mask)
            assert got.shape[0] == len(au.selected(cond_mask, table_mask))
            k += 1


# ---- ADD semantics ----------------------------------------------------------------------------------------------

def test_two_bands_cut_inside_a_cell_row_add_up_to_one_call(scene, tables):
    inp = inputs(("grid", 1041), 1041, ROWS, 25, 70 + 1041, tables)
    sc = scene(inp)
    for (wx, wy), name in (((8, 25), "random"), ((100, 25.6), "all 65535")):
        cellx, celly = maps(1041, ROWS, wx, wy, (5, 3), (3, 2))
        whole = check_weighted(sc, cellx, celly, WEIGHTS[name])
        cut = 31
        assert celly[cut - 1] == celly[cut] >= 0                 # the cut lies inside a cell row
        parts = check_weighted(sc, cellx, celly, WEIGHTS[name], bands=[(0, cut), (cut, ROWS - cut)])
        np.testing.assert_array_equal(parts, whole)


def test_a_second_call_doubles_every_triple(scene, tables):
    inp = inputs(("grid", 1041), 1041, ROWS, 25, 70 + 1041, tables)
    sc = scene(inp)
    cellx, celly = maps(1041, ROWS, 17.3, 15.9, (5, 3), (3, 2))
    once = check_weighted(sc, cellx, celly, Q50)
    twice = run_weighted(sc, cellx, celly, Q50, repeat=2)
    np.testing.assert_array_equal(twice, 2 * once)
    assert once[..., 1].max() > 0 and once[..., 2].max() > 0


# ---- grid_finish_weighted -------------------------------------------------------------------------------------------

def test_finish_on_hand_made_triples(engine, tables):
    engine.set_tables(tables)
    triples = hand_made_triples(Q50)
    acc = np.array([triples, triples[::-1]], np.int64)
    idx = [0, len(triples) - 1, 3, 3, 0]
    means, cnq, shared = run_finish_weighted(engine, acc, idx, Q50)
    want = [ru.cn(*tr, Q50) for tr in triples]
    assert cnq[0].tolist() == want and cnq[1].tolist() == want[::-1]
    assert want == [host.runoff_cn(*tr, Q50) for tr in triples]
    np.testing.assert_array_equal(means, gu.means(acc[..., :2]))
    np.testing.assert_array_equal(shared, acc[:, idx, :])
    means, cnq, shared = run_finish_weighted(engine, acc, [], Q50)         # n_shared = 0: no pointer is touched
    assert cnq[0].tolist() == want and shared.shape == (2, 0, 3)
    # a table that goes down somewhere: the smallest c all the same
    w = Q50.copy()
    w[40:60] = w[40:60][::-1]
    _means, cnq, _shared = run_finish_weighted(engine, acc, [], w)
    assert cnq[0].tolist() == [ru.cn(*tr, w) for tr in triples]


def test_finish_on_the_sums_of_a_scene(scene, tables):
    inp = inputs(("grid", 1041), 1041, ROWS, 25, 70 + 1041, tables)
    sc = scene(inp)
    cellx, celly = maps(1041, ROWS, 8, 8, (5, 3), (3, 2))
    acc = check_weighted(sc, cellx, celly, Q50)
    n, sw = acc[..., 1], acc[..., 2]
    want = ru.cn_array(acc, Q50)
    m = gu.means(acc[..., :2])
    assert (n == 0).any() and ((n > 0) & (sw == 0)).any() and (sw > 0).any()       # the scene holds all of it
    assert ((sw > 0) & (want > m)).any()                    # the composite lies above the mean somewhere
    flat = acc.reshape(18, -1, 3)
    n_cells = flat.shape[1]
    idx = [0, n_cells - 1, 7, 7, n_cells // 2]
    means, cnq, shared = run_finish_weighted(sc.eng, flat, idx, Q50)
    np.testing.assert_array_equal(means, gu.means(flat[..., :2]))
    np.testing.assert_array_equal(cnq, want.reshape(18, -1))
    np.testing.assert_array_equal(shared, flat[:, idx, :])
    assert (cnq[n.reshape(18, -1) == 0] == 255).all()


# ---- state and errors -----------------------------------------------------------------------------------------------

def _sums(eng, esa, cj, cx, cy, acc, W=32, rows=4, ncx=2, ncy=1, cond=3, table=0x1FF):
    rc = gpu.lib().gcn10_gpu_grid_sums_weighted(eng._ctx, esa, W, rows, cj, cx, cy, ncx, ncy, cond, table, acc, None)
    return rc, gpu.lib().gcn10_gpu_last_error().decode()


def test_state_and_errors(tables):
    eng = gpu.Engine(0)
    L = gpu.lib()
    try:
        inp = Inputs(32, 4, 8, 3, tables)
        cellx, celly = (np.arange(32) // 16).astype(np.int32), np.zeros(4, np.int32)
        bufs = [eng.upload(a) for a in (inp.esa, inp.coarse, inp.ci, inp.cj, cellx, celly)]
        nbytes = 18 * 2 * 24
        acc = eng.alloc(nbytes)
        out = eng.alloc(256)
        eng.memset(acc.ptr, POISON, nbytes)
        eng.memset(out.ptr, POISON, 256)
        esa, cj, cx, cy = bufs[0].ptr, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr
        finish = (acc.ptr, 18, 2, out.ptr, out.ptr + 64, None, 0, None)
        w = np.ascontiguousarray(Q50)
        # weights need tables; the weighted calls need weights, and new ones after every set_tables
        rc = L.gcn10_gpu_set_weights(eng._ctx, w.ctypes.data)
        assert rc == E_STATE and "gcn10_gpu_set_tables" in L.gcn10_gpu_last_error().decode()
        eng.set_tables(tables)
        eng.prepare_tile(bufs[1].ptr, inp.hsx, inp.hsy, bufs[2].ptr, 32)
        for _round in range(2):
            rc, msg = _sums(eng, esa, cj, cx, cy, acc.ptr)
            assert rc == E_STATE and "gcn10_gpu_set_weights" in msg, (rc, msg)
            rc = L.gcn10_gpu_grid_finish_weighted(eng._ctx, *finish, None)
            assert rc == E_STATE and "gcn10_gpu_set_weights" in L.gcn10_gpu_last_error().decode()
            rc = L.gcn10_gpu_set_weights(eng._ctx, None)
            assert rc == E_INVAL and "gcn10_gpu_set_weights" in L.gcn10_gpu_last_error().decode()
            eng.set_weights(w)
            rc, msg = _sums(eng, esa, cj, cx, cy, acc.ptr, W=48)
            assert rc == E_STATE and "prepare" in msg, (rc, msg)
            eng.set_tables(tables)                      # invalidates the weights (the prepared tile stays)
        eng.set_weights(w)
        bad = [dict(rows=0), dict(rows=-1), dict(ncx=0), dict(ncx=-2), dict(ncy=0), dict(ncy=-1), dict(cond=0),
               dict(cond=4), dict(table=0), dict(table=1 << 9), dict(cx=None), dict(cy=None), dict(acc=None)]
        for kw in bad:
            args = dict(cx=cx, cy=cy, acc=acc.ptr)
            args.update(kw)
            rc, msg = _sums(eng, esa, cj, **args)
            assert rc == E_INVAL and "gcn10_gpu_grid_sums_weighted" in msg, (kw, rc, msg)
        o = out.ptr
        for args in ((acc.ptr, 0, 2, o, o + 64, None, 0, None), (acc.ptr, 19, 2, o, o + 64, None, 0, None),
                     (acc.ptr, 18, 0, o, o + 64, None, 0, None), (None, 18, 2, o, o + 64, None, 0, None),
                     (acc.ptr, 18, 2, None, o + 64, None, 0, None), (acc.ptr, 18, 2, o, None, None, 0, None),
                     (acc.ptr, 18, 2, o, o + 64, None, 1, acc.ptr), (acc.ptr, 18, 2, o, o + 64, cx, 1, None)):
            rc = L.gcn10_gpu_grid_finish_weighted(eng._ctx, *args, None)
            assert rc == E_INVAL and "gcn10_gpu_grid_finish_weighted" in L.gcn10_gpu_last_error().decode(), args
        eng.sync()
        assert (eng.download(acc.ptr, (nbytes,)) == POISON).all(), "a refused call wrote"
        assert (eng.download(out.ptr, (256,)) == POISON).all(), "a refused call wrote"
        # and the good call, after all that
        eng.memset(acc.ptr, 0, nbytes)
        rc, msg = _sums(eng, esa, cj, cx, cy, acc.ptr)
        assert rc == OK, msg
        eng.sync()
        got = eng.download(acc.ptr, (nbytes,)).view(np.uint64).astype(np.int64).reshape(18, 1, 2, 3)
        want = np.zeros((18, 1, 2, 3), np.int64)
        for r in range(18):
            ru.add_triples(want[r], au.oracle_rasters(inp.esa, inp.soil, tables, [r])[r], cellx, celly, Q50)
        np.testing.assert_array_equal(got, want)
    finally:
        eng.sync()
        eng.close()
