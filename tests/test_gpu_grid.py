"""GPU: the sums and means on a model grid (gcn10_gpu_grid_sums, gcn10_gpu_grid_finish) through the ABI face.  Needs
an MI355X.

Inputs: the recipe of tests/test_gpu_aggregate.py (patchy landcover with noise, the awkward landcover and soil values,
a cj that repeats and goes back).  Expected values: the oracle's full-resolution rasters (tests/aggutil.py::
oracle_rasters), accumulated in numpy int64 with np.add.at over maps this file builds itself (tests/gridutil.py::
add_sums).  Every comparison is bit-exact, on the pairs and on the means.  Shapes are the smallest at which the kernel
can go wrong: widths around a 16-pixel column group, above the 4096 columns of a workgroup and the 36001 of a block (nine
chunks; expected sums by np.bincount there, tests/gridutil.py), cells of 8 pixels (three
cell columns in one group) to one cell wider than the strip, rows of less than a cell to several of them, -1 runs that
end inside a group, landcover one byte into its allocation.
"""
import ctypes as C

import numpy as np
import pytest

from gcn10_amd import gpu
from tests import aggutil as au
from tests import gridutil as gu
from tests.test_gpu_aggregate import Inputs, inputs, scene  # noqa: F401  (the recipe, its cache and the fixture)
from tests.util import random_tables

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_STATE = 0, -1, -4
POISON = 0xA5
GUARD = 256
ROWS = 60
WIDTHS = [1, 15, 16, 17, 1039, 1041, 2064, 4200, 36001]    # 36001: nine chunks, a last group of one pixel
# (cell width, cell height) in pixels: every width and every height of 8, 8.5, 15.9, 16, 17.3, 25, 25.6, 100 and "wider
# than the strip" once; heights of 100 (fewer rows than one cell), 60 (exactly one) and 24 (2.5 cell rows) as well
CELLS = [(8, 8), (8.5, 100), (15.9, 24), (16, 60), (17.3, 17.3), (25, 25.6), (25.6, 8.5), (100, 15.9), (1e6, 16),
         (24, 1e6), (60, 25)]
WORKGROUP_PX = 4096     # columns of a workgroup of the kernel: a cell wider than that is summed by several


def maps(W, rows, wx, wy, lead=(0, 0), trail=(0, 0), off=(0.3, 0.6)):
    """int32 cell column of every column and cell row of every row for cells of wx x wy pixels whose first edge lies
    `off` pixels before column / row `lead`; -1 for the first `lead` and the last `trail` of them."""
    out = []
    for n, w, a, b, o in ((W, wx, lead[0], trail[0], off[0]), (rows, wy, lead[1], trail[1], off[1])):
        i = np.arange(n)
        k = np.floor((i - a + o) / w).astype(np.int64)
        k = np.where((i >= a) & (i < n - b), k, -1)
        if (k >= 0).any():
            k = np.where(k >= 0, k - k[k >= 0].min(), -1)
        out.append(k.astype(np.int32))
    return out


def cells_in_a_group(cellx):
    """the most different cell columns among 16 columns from a multiple of 16 on"""
    return max(len(set(cellx[g:g + 16][cellx[g:g + 16] >= 0].tolist())) for g in range(0, len(cellx), 16))


def run_sums(sc, cellx, celly, cond_mask=3, table_mask=0x1FF, bands=None, repeat=1):
    """int64[n_sel][ncy][ncx][2] after grid_sums over the scene's strip -- in one call, or one call per (y0, rows) of
    `bands` --, `repeat` times; asserts that not a byte around the pairs was written."""
    inp, eng = sc.inp, sc.eng
    sel = au.selected(cond_mask, table_mask)
    ncx, ncy = int(cellx.max()) + 1, int(celly.max()) + 1
    nbytes = len(sel) * ncy * ncx * 16
    buf = eng.alloc(nbytes + 2 * GUARD)
    ups = [eng.upload(cellx), eng.upload(celly)]
    try:
        eng.memset(buf.ptr, POISON, nbytes + 2 * GUARD)
        eng.memset(buf.ptr + GUARD, 0, nbytes)
        for _rep in range(repeat):
            for y0, n in bands or [(0, len(celly))]:
                eng.grid_sums(sc.esa_ptr + y0 * inp.W, inp.W, n, sc.bufs[3].ptr + 4 * y0, ups[0].ptr, ups[1].ptr + 4 * y0,
                              ncx, ncy, cond_mask, table_mask, buf.ptr + GUARD)
        eng.sync()
        img = eng.download(buf.ptr, (nbytes + 2 * GUARD,))
    finally:
        eng.sync()
        for b in [buf] + ups:
            b.close()
    assert (img[:GUARD] == POISON).all() and (img[GUARD + nbytes:] == POISON).all(), "bytes around acc were written"
    return img[GUARD:GUARD + nbytes].view(np.uint64).astype(np.int64).reshape(len(sel), ncy, ncx, 2)


def want_sums(inp, cellx, celly, cond_mask=3, table_mask=0x1FF):
    sel = au.selected(cond_mask, table_mask)
    acc = np.zeros((len(sel), int(celly.max()) + 1, int(cellx.max()) + 1, 2), np.int64)
    for q, r in enumerate(sel):
        gu.add_sums(acc[q], inp.want(r)[:len(celly)], cellx, celly)
    return acc


def check_sums(sc, cellx, celly, cond_mask=3, table_mask=0x1FF, **kw):
    got = run_sums(sc, cellx, celly, cond_mask, table_mask, **kw)
    want = want_sums(sc.inp, cellx, celly, cond_mask, table_mask)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "W=%d: %d of %d words differ, first (q, cy, cx, word) = %s: got %d, want %d" % (
        sc.inp.W, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    return got


def run_finish(eng, acc, shared_idx):
    """(means uint8[n_sel][n_cells], shared int64[n_sel][n_shared][2]) of grid_finish over int64 pairs
    [n_sel][n_cells][2]; asserts that not a byte around means and shared was written."""
    n_sel, n_cells = acc.shape[:2]
    idx = np.asarray(shared_idx, np.uint32)
    n_sh = len(idx)
    d_acc = eng.upload(acc.astype(np.uint64))
    d_idx = eng.upload(idx) if n_sh else None
    means = eng.alloc(n_sel * n_cells + 2 * GUARD)
    shared = eng.alloc(n_sel * n_sh * 16 + 2 * GUARD)
    try:
        eng.memset(means.ptr, POISON, means.nbytes)
        eng.memset(shared.ptr, POISON, shared.nbytes)
        eng.grid_finish(d_acc.ptr, n_sel, n_cells, means.ptr + GUARD, d_idx.ptr if n_sh else None, n_sh,
                        shared.ptr + GUARD if n_sh else None)
        eng.sync()
        m = eng.download(means.ptr, (means.nbytes,))
        s = eng.download(shared.ptr, (shared.nbytes,))
    finally:
        eng.sync()
        for b in (d_acc, d_idx, means, shared):
            if b is not None:
                b.close()
    assert (m[:GUARD] == POISON).all() and (m[GUARD + n_sel * n_cells:] == POISON).all(), "bytes around means"
    assert (s[:GUARD] == POISON).all() and (s[GUARD + n_sel * n_sh * 16:] == POISON).all(), "bytes around shared"
    return (m[GUARD:GUARD + n_sel * n_cells].reshape(n_sel, n_cells),
            s[GUARD:GUARD + n_sel * n_sh * 16].view(np.uint64).astype(np.int64).reshape(n_sel, n_sh, 2))


# ---- widths, cell sizes, maps --------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", WIDTHS)
def test_every_width_and_cell_size_equals_the_summed_oracle(scene, tables, W):
    inp = inputs(("grid", W), W, ROWS, 25, 70 + W, tables)
    sc = scene(inp)                                         # landcover one byte into its allocation
    # the wide strips take the small cells, the large ones and the single cell; the others every pair
    cells = CELLS if W <= 1041 else [CELLS[0], CELLS[5], CELLS[8]]
    most = widest = 0
    for wx, wy in cells:
        lead, trail = ((5, 3), (3, 2)) if W > 30 else ((0, 0), (0, 0))
        cellx, celly = maps(W, ROWS, wx, wy, lead, trail)
        check_sums(sc, cellx, celly)
        most = max(most, cells_in_a_group(cellx))
        widest = max(widest, int(np.bincount(cellx[cellx >= 0]).max()))
    if W >= 1039:
        assert most == 3                # cells of 8 pixels: three cell columns in one 16-pixel group
    if W == 4200:
        assert widest > WORKGROUP_PX    # one cell summed by two workgroups' columns (and by several bands of rows)


def test_the_shapes_reach_both_regimes():
    """What the comparison above relies on, from the shapes alone (no GPU work)."""
    cellx, celly = maps(1041, ROWS, 8, 8, (5, 3), (3, 2))
    assert cells_in_a_group(cellx) == 3 and (cellx[:5] == -1).all() and cellx[5] == 0 and (cellx[-3:] == -1).all()
    assert (celly[:3] == -1).all() and (celly[-2:] == -1).all() and celly.max() >= 6
    cellx, celly = maps(4200, ROWS, 1e6, 16, (5, 3), (3, 2))
    assert cellx.max() == 0 and (cellx == 0).sum() > WORKGROUP_PX
    # rows: fewer than one cell, exactly one, two and a half
    assert maps(16, ROWS, 8, 100)[1].max() == 0 and maps(16, ROWS, 8, 60, off=(0, 0))[1].max() == 0
    assert np.bincount(maps(16, ROWS, 8, 24, off=(0, 0))[1]).tolist() == [24, 24, 12]


@pytest.mark.parametrize("lead", [1, 15, 16, 21, 37])
def test_a_run_of_minus_one_that_ends_inside_a_column_group(scene, tables, lead):
    inp = inputs(("grid", 1041), 1041, ROWS, 25, 70 + 1041, tables)
    sc = scene(inp)
    for wx, wy in ((8, 8), (25.6, 17.3)):
        cellx, celly = maps(1041, ROWS, wx, wy, (lead, lead % 7), (lead + 2, 1))
        check_sums(sc, cellx, celly)
    # -1 everywhere but one column and one row
    cellx, celly = np.full(1041, -1, np.int32), np.full(ROWS, -1, np.int32)
    cellx[lead], celly[lead % ROWS] = 0, 0
    got = check_sums(sc, cellx, celly)
    assert got.shape == (18, 1, 1, 2) and got[..., 1].max() <= 1


@pytest.mark.parametrize("offset", [0, 1, 3])
def test_landcover_at_any_byte_offset(scene, tables, offset):
    inp = inputs(("grid", 1041), 1041, ROWS, 25, 70 + 1041, tables)
    sc = scene(inp, offset=offset)
    check_sums(sc, *maps(1041, ROWS, 25.6, 25.6, (5, 3), (3, 2)))
    check_sums(sc, *maps(1041, ROWS, 8.5, 8, (0, 0), (0, 0)))


@pytest.mark.parametrize("n_tables", [9, 5])
def test_awkward_tables_and_mask_subsets(scene, n_tables):
    t = random_tables(5, n_tables)
    inp = inputs(("grid nasty", n_tables), 333, 77, 25, 41, t)
    sc = scene(inp)
    full = (1 << n_tables) - 1
    cellx, celly = maps(333, 77, 8.5, 8, (2, 1), (1, 2))
    for cond_mask in (1, 2, 3):
        for table_mask in (full, 1, 1 << (n_tables - 1), 0x15 & full):     # all, one raster per condition, a subset
            got = check_sums(sc, cellx, celly, cond_mask, table_mask)
            assert got.shape[0] == len(au.selected(cond_mask, table_mask))


# ---- ADD semantics ----------------------------------------------------------------------------------------------

def test_two_bands_cut_inside_a_cell_row_add_up_to_one_call(scene, tables):
    inp = inputs(("grid", 1041), 1041, ROWS, 25, 70 + 1041, tables)
    sc = scene(inp)
    for wx, wy in ((8, 25), (100, 25.6)):
        cellx, celly = maps(1041, ROWS, wx, wy, (5, 3), (3, 2))
        whole = check_sums(sc, cellx, celly)
        cut = 31
        assert celly[cut - 1] == celly[cut] >= 0                 # the cut lies inside a cell row
        parts = check_sums(sc, cellx, celly, bands=[(0, cut), (cut, ROWS - cut)])
        np.testing.assert_array_equal(parts, whole)


def test_a_second_call_doubles_every_pair(scene, tables):
    inp = inputs(("grid", 1041), 1041, ROWS, 25, 70 + 1041, tables)
    sc = scene(inp)
    cellx, celly = maps(1041, ROWS, 17.3, 15.9, (5, 3), (3, 2))
    once = check_sums(sc, cellx, celly)
    twice = run_sums(sc, cellx, celly, repeat=2)
    np.testing.assert_array_equal(twice, 2 * once)
    assert once[..., 1].max() > 0


# ---- grid_finish ---------------------------------------------------------------------------------------------------

def test_finish_on_hand_made_pairs(engine):
    """n = 0 -> 255; exact halves round up; sums beyond 32 bits."""
    pairs = [(0, 0), (5, 2), (7, 2), (1, 3), (1, 2), (254 << 31, 1 << 31), (3 * (1 << 40) + (1 << 39), 1 << 40),
             (100, 1), (0, 7)]
    want = [255, 3, 4, 0, 1, 254, 4, 100, 0]
    acc = np.array([pairs, pairs[::-1]], np.int64)
    idx = [0, len(pairs) - 1, 3, 3, 0]
    means, shared = run_finish(engine, acc, idx)
    assert means[0].tolist() == want and means[1].tolist() == want[::-1]
    np.testing.assert_array_equal(shared, acc[:, idx, :])
    means, shared = run_finish(engine, acc, [])            # n_shared = 0: no pointer is touched
    assert means[0].tolist() == want and shared.shape == (2, 0, 2)


def test_finish_on_the_sums_of_a_scene(scene, tables):
    inp = inputs(("grid", 1041), 1041, ROWS, 25, 70 + 1041, tables)
    sc = scene(inp)
    cellx, celly = maps(1041, ROWS, 8, 8, (5, 3), (3, 2))
    acc = check_sums(sc, cellx, celly)
    s, n = acc[..., 0], acc[..., 1]
    ties = (n > 0) & ((2 * s + n) % (2 * np.maximum(n, 1)) == 0)
    assert (n == 0).any() and ties.any() and ((n > 0) & (n < 64)).any()    # the scene holds all of it
    flat = acc.reshape(18, -1, 2)
    n_cells = flat.shape[1]
    idx = [0, n_cells - 1, 7, 7, n_cells // 2]
    means, shared = run_finish(sc.eng, flat, idx)
    np.testing.assert_array_equal(means, gu.means(flat))
    np.testing.assert_array_equal(shared, flat[:, idx, :])
    assert (means[n.reshape(18, -1) == 0] == 255).all()


@pytest.mark.parametrize("f", [16, 25])
def test_cells_of_f_pixels_equal_the_area_means(scene, tables, f):
    """A cross-check between two GPU paths, not the parity claim (that is the oracle's, above)."""
    inp = inputs(("grid", 1041), 1041, ROWS, 25, 70 + 1041, tables)
    sc = scene(inp)
    eng = sc.eng
    x0, x1 = 5, 1038
    i = np.arange(1041)
    cellx = np.where((i >= x0) & (i < x1), (i - x0) // f, -1).astype(np.int32)
    celly = (np.arange(ROWS) // f).astype(np.int32)
    acc = check_sums(sc, cellx, celly)
    Wa, Ha = au.cells(x1 - x0, f), au.cells(ROWS, f)
    means, _ = run_finish(eng, acc.reshape(18, -1, 2), [])
    out = eng.alloc(18 * Wa * Ha)
    try:
        eng.aggregate(sc.esa_ptr, 1041, ROWS, sc.bufs[3].ptr, x0, x1, f, 3, 0x1FF,
                      [out.ptr + q * Wa * Ha for q in range(18)], Wa)
        eng.sync()
        agg = eng.download(out.ptr, (18, Wa * Ha))
    finally:
        eng.sync()
        out.close()
    np.testing.assert_array_equal(means, agg)


# ---- errors -------------------------------------------------------------------------------------------------------

def _sums(eng, esa, cj, cx, cy, acc, W=32, rows=4, ncx=2, ncy=1, cond=3, table=0x1FF):
    rc = gpu.lib().gcn10_gpu_grid_sums(eng._ctx, esa, W, rows, cj, cx, cy, ncx, ncy, cond, table, acc, None)
    return rc, gpu.lib().gcn10_gpu_last_error().decode()


def test_errors(tables):
    eng = gpu.Engine(0)
    try:
        inp = Inputs(32, 4, 8, 3, tables)
        cellx, celly = (np.arange(32) // 16).astype(np.int32), np.zeros(4, np.int32)
        bufs = [eng.upload(a) for a in (inp.esa, inp.coarse, inp.ci, inp.cj, cellx, celly)]
        nbytes = 18 * 2 * 16
        acc = eng.alloc(nbytes)
        eng.memset(acc.ptr, POISON, nbytes)
        esa, cj, cx, cy = bufs[0].ptr, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr
        rc, msg = _sums(eng, esa, cj, cx, cy, acc.ptr)
        assert rc == E_STATE and "gcn10_gpu_set_tables" in msg, (rc, msg)
        eng.set_tables(tables)
        rc, msg = _sums(eng, esa, cj, cx, cy, acc.ptr)
        assert rc == E_STATE and "prepare" in msg, (rc, msg)
        eng.prepare_tile(bufs[1].ptr, inp.hsx, inp.hsy, bufs[2].ptr, 32)
        rc, msg = _sums(eng, esa, cj, cx, cy, acc.ptr, W=48)
        assert rc == E_STATE and "prepare" in msg, (rc, msg)
        bad = [dict(rows=0), dict(rows=-1), dict(ncx=0), dict(ncx=-2), dict(ncy=0), dict(ncy=-1), dict(cond=0),
               dict(cond=4), dict(table=0), dict(table=1 << 9), dict(cx=None), dict(cy=None), dict(acc=None)]
        for kw in bad:
            args = dict(cx=cx, cy=cy, acc=acc.ptr)
            args.update(kw)
            rc, msg = _sums(eng, esa, cj, **args)
            assert rc == E_INVAL and "gcn10_gpu_grid_sums" in msg, (kw, rc, msg)
        L = gpu.lib()
        means = eng.alloc(64)
        for args in ((acc.ptr, 0, 2, means.ptr, None, 0, None), (acc.ptr, 19, 2, means.ptr, None, 0, None),
                     (acc.ptr, 18, 0, means.ptr, None, 0, None), (None, 18, 2, means.ptr, None, 0, None),
                     (acc.ptr, 18, 2, None, None, 0, None), (acc.ptr, 18, 2, means.ptr, None, 1, acc.ptr),
                     (acc.ptr, 18, 2, means.ptr, cx, 1, None)):
            rc = L.gcn10_gpu_grid_finish(eng._ctx, *args, None)
            assert rc == E_INVAL and "gcn10_gpu_grid_finish" in L.gcn10_gpu_last_error().decode(), args
        eng.sync()
        assert (eng.download(acc.ptr, (nbytes,)) == POISON).all(), "a refused call wrote"
        eng.memset(acc.ptr, 0, nbytes)
        rc, msg = _sums(eng, esa, cj, cx, cy, acc.ptr)
        assert rc == OK, msg
        eng.sync()
        got = eng.download(acc.ptr, (nbytes,)).view(np.uint64).astype(np.int64).reshape(18, 1, 2, 2)
        want = np.zeros((18, 1, 2, 2), np.int64)
        for r in range(18):
            gu.add_sums(want[r], au.oracle_rasters(inp.esa, inp.soil, tables, [r])[r], cellx, celly)
        np.testing.assert_array_equal(got, want)
    finally:
        eng.sync()
        eng.close()
