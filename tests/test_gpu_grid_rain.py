"""GPU: the sums on a model grid with a weight table per cell (gcn10_gpu_set_rain_tables, gcn10_gpu_grid_sums_rain,
gcn10_gpu_grid_finish_rain) through the ABI face.  Needs an MI355X.

Inputs: the recipe of tests/test_gpu_aggregate.py (the landcover one byte into its allocation, so that its last byte
is the allocation's last) and maps this file builds.  Expected values: the oracle's full-resolution rasters summed per
cell in numpy with the table the cell's byte names, and runoffutil.cn per cell (tests/rainutil.py); with a constant
field also the triples and bytes of gcn10_gpu_grid_sums_weighted / _finish_weighted for the same table, a cross-check
between two GPU paths.  Every comparison is bit for bit.  The shapes follow the kernel's items, whose size is read
from the library (gpu.grid_rain_item): cells of 8 pixels, cells of 25 and 26 pixels in turn, cells cut by items, one
cell over several items each way, a last column group of one pixel.  Every strip here is short enough for the launch
to stay at its floor of 16 rows per item; items of 17 to 127 rows, the full 512 x 127 of a block-sized call among them,
are run in tests/test_gpu_capped_grids.py ("6. grid_sums_rain").
"""
import numpy as np
import pytest

from gcn10_amd import gpu, host
from tests import aggutil as au
from tests import rainutil as rn
from tests import runoffutil as ru
from tests import stormutil
from tests.test_gpu_aggregate import Inputs, inputs, scene  # noqa: F401  (the recipe, its cache and the fixture)
from tests.test_gpu_grid import GUARD, POISON, maps, run_sums
from tests.test_gpu_grid_runoff import run_finish_weighted, run_weighted
from tests.test_runoff_host import hand_made_triples

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_STATE = 0, -1, -4
INT_MIN = -2 ** 31
TABLES = rn.tables_256()
Q50 = ru.table(50, 0.2)
CONSTANT = {"50 mm": Q50}
CONSTANT.update({name: stormutil.POOL[name] for name in stormutil.ADVERSARIAL})
W1, ROWS1 = 1043, 61


def field_for(ncx, ncy, seed=3):
    """uint8[ncy][ncx], random, with all 256 values where there are 256 cells"""
    f = np.random.default_rng(seed).integers(0, 256, (ncy, ncx)).astype(np.uint8)
    if f.size >= 256:
        f.reshape(-1)[np.random.default_rng(seed + 1).permutation(f.size)[:256]] = np.arange(256, dtype=np.uint8)
        assert len(np.unique(f)) == 256
    return f


def map_of(n, sizes, lead, trail):
    """int32[n]: -1 for the first `lead` and the last `trail` entries, between them cells of sizes[0], sizes[1], ...
    entries, round and round"""
    m = np.full(n, -1, np.int32)
    at, k = lead, 0
    while at < n - trail:
        size = min(sizes[k % len(sizes)], n - trail - at)
        m[at:at + size] = k
        at, k = at + size, k + 1
    return m


def run_rain(sc, cellx, celly, field, tables, cond_mask=3, table_mask=0x1FF, bands=None, repeat=1):
    """int64[n_sel][ncy][ncx][3] after set_rain_tables(tables) and grid_sums_rain over the scene's strip with the field
    uint8[ncy][ncx] -- in one call, or one call per (y0, rows) of `bands` --, `repeat` times; asserts that not a byte
    around the triples was written."""
    inp, eng = sc.inp, sc.eng
    sel = au.selected(cond_mask, table_mask)
    ncy, ncx = field.shape
    nbytes = len(sel) * ncy * ncx * 24
    buf = eng.alloc(nbytes + 2 * GUARD)
    ups = [eng.upload(np.ascontiguousarray(cellx, np.int32)), eng.upload(np.ascontiguousarray(celly, np.int32)),
           eng.upload(np.ascontiguousarray(field))]
    try:
        eng.set_rain_tables(tables)
        eng.memset(buf.ptr, POISON, nbytes + 2 * GUARD)
        eng.memset(buf.ptr + GUARD, 0, nbytes)
        for _rep in range(repeat):
            for y0, n in bands or [(0, len(celly))]:
                eng.grid_sums_rain(sc.esa_ptr + y0 * inp.W, inp.W, n, sc.bufs[3].ptr + 4 * y0, ups[0].ptr,
                                   ups[1].ptr + 4 * y0, ncx, ncy, cond_mask, table_mask, ups[2].ptr, buf.ptr + GUARD)
        eng.sync()
        img = eng.download(buf.ptr, (nbytes + 2 * GUARD,))
    finally:
        eng.sync()
        for b in [buf] + ups:
            b.close()
    assert (img[:GUARD] == POISON).all() and (img[GUARD + nbytes:] == POISON).all(), "bytes around acc were written"
    return img[GUARD:GUARD + nbytes].view(np.uint64).astype(np.int64).reshape(len(sel), ncy, ncx, 3)


def want_rain(inp, cellx, celly, field, tables, cond_mask=3, table_mask=0x1FF):
    sel = au.selected(cond_mask, table_mask)
    acc = np.zeros((len(sel),) + field.shape + (3,), np.int64)
    for q, r in enumerate(sel):
        rn.add_triples(acc[q], inp.want(r)[:len(celly)], cellx, celly, field, tables)
    return acc


def check_rain(sc, cellx, celly, field, tables=TABLES, cond_mask=3, table_mask=0x1FF, **kw):
    got = run_rain(sc, cellx, celly, field, tables, cond_mask, table_mask, **kw)
    want = want_rain(sc.inp, cellx, celly, field, tables, cond_mask, table_mask)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "W=%d: %d of %d words differ, first (q, cy, cx, word) = %s: got %d, want %d" % (
        sc.inp.W, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    return got


def run_finish_rain(eng, acc, field, tables, shared_idx):
    """(means, cnq uint8[n_sel][n_cells], shared int64[n_sel][n_shared][3]) of set_rain_tables(tables) and
    grid_finish_rain over int64 triples [n_sel][n_cells][3] with field uint8[n_cells]; asserts that not a byte around
    the three was written."""
    n_sel, n_cells = acc.shape[:2]
    idx = np.asarray(shared_idx, np.uint32)
    n_sh, nb = len(idx), n_sel * n_cells
    d_acc = eng.upload(acc.astype(np.uint64))
    d_field = eng.upload(np.ascontiguousarray(field, np.uint8).reshape(n_cells))
    d_idx = eng.upload(idx) if n_sh else None
    out = [eng.alloc(nb + 2 * GUARD), eng.alloc(nb + 2 * GUARD), eng.alloc(n_sel * n_sh * 24 + 2 * GUARD)]
    try:
        eng.set_rain_tables(tables)
        for b in out:
            eng.memset(b.ptr, POISON, b.nbytes)
        eng.grid_finish_rain(d_acc.ptr, n_sel, n_cells, d_field.ptr, out[0].ptr + GUARD, out[1].ptr + GUARD,
                             d_idx.ptr if n_sh else None, n_sh, out[2].ptr + GUARD if n_sh else None)
        eng.sync()
        img = [eng.download(b.ptr, (b.nbytes,)) for b in out]
    finally:
        eng.sync()
        for b in [d_acc, d_field, d_idx] + out:
            if b is not None:
                b.close()
    for name, im in zip(("means", "cnq", "shared"), img):
        assert (im[:GUARD] == POISON).all() and (im[-GUARD:] == POISON).all(), "bytes around %s were written" % name
    return (img[0][GUARD:-GUARD].reshape(n_sel, n_cells), img[1][GUARD:-GUARD].reshape(n_sel, n_cells),
            img[2][GUARD:-GUARD].view(np.uint64).astype(np.int64).reshape(n_sel, n_sh, 3))


def strip(scene, tables):
    return scene(inputs(("rain", W1), W1, ROWS1, 25, 9 + W1, tables))


# ---- a constant field: the weighted calls' words and bytes ----------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CONSTANT))
def test_a_constant_field_equals_the_weighted_calls(scene, tables, name):
    """Table 2 of three is `name`, every cell's byte is 2: words 0, 1 and 2 of gcn10_gpu_grid_sums_weighted with that
    table, and the means and runoff-equivalent bytes of gcn10_gpu_grid_finish_weighted."""
    sc = strip(scene, tables)
    w = CONSTANT[name]
    three = np.stack([TABLES[7], TABLES[200], w])
    for wx, wy in ((8, 8), (25, 25.6)):
        cellx, celly = maps(W1, ROWS1, wx, wy, (5, 3), (3, 2))
        ncx, ncy = int(cellx.max()) + 1, int(celly.max()) + 1
        field = np.full((ncy, ncx), 2, np.uint8)
        got = run_rain(sc, cellx, celly, field, three)
        np.testing.assert_array_equal(got, run_weighted(sc, cellx, celly, w))
        np.testing.assert_array_equal(got[..., :2], run_sums(sc, cellx, celly))
        flat = got.reshape(18, -1, 3)
        means, cnq, _ = run_finish_rain(sc.eng, flat, field, three, [])
        w_means, w_cnq, _ = run_finish_weighted(sc.eng, flat, [], w)
        np.testing.assert_array_equal(means, w_means)
        np.testing.assert_array_equal(cnq, w_cnq)


# ---- a random field, 256 tables, against the restatement ------------------------------------------------------------

def test_one_cell_and_a_last_group_of_one_pixel(scene, tables):
    sc = scene(inputs(("rain", 17), 17, 17, 25, 26, tables))
    cellx, celly = maps(17, 17, 1e6, 1e6)
    assert cellx.max() == 0 and celly.max() == 0
    for b in (0, 3, 255):
        got = check_rain(sc, cellx, celly, np.full((1, 1), b, np.uint8))
        assert got.shape == (18, 1, 1, 3) and got[..., 1].max() > 0


CELLS_1043 = {
    "8 x 8, the floor": lambda: maps(W1, ROWS1, 8, 8, (5, 3), (3, 2)),
    "25 and 26 in turn": lambda: (map_of(W1, (25, 26), 5, 3), map_of(ROWS1, (25, 26), 3, 2)),
    "26 and 25 in turn": lambda: (map_of(W1, (26, 25), 5, 3), map_of(ROWS1, (26, 25), 3, 2)),
    "120 x 50": lambda: maps(W1, ROWS1, 120, 50, (5, 3), (3, 2)),
    "one cell over everything": lambda: maps(W1, ROWS1, 1e6, 1e6, (5, 3), (3, 2)),
}


@pytest.mark.parametrize("cells", sorted(CELLS_1043))
def test_a_random_field_equals_the_summed_oracle(scene, tables, cells):
    """-1 columns and rows on all four sides, the landcover at an odd byte offset; both conditions, one, one raster."""
    sc = strip(scene, tables)
    assert sc.esa_ptr % 2 == 1
    cellx, celly = CELLS_1043[cells]()
    assert (cellx[:5] == -1).all() and (cellx[-3:] == -1).all() and (celly[:3] == -1).all() and (celly[-2:] == -1).all()
    ncx, ncy = int(cellx.max()) + 1, int(celly.max()) + 1
    field = field_for(ncx, ncy)
    if cells.startswith("8 x 8"):
        assert len(np.unique(field)) == 256
    got = check_rain(sc, cellx, celly, field)
    assert got.shape == (18, ncy, ncx, 3) and got[..., 2].max() > 0
    check_rain(sc, cellx, celly, field, cond_mask=2)
    check_rain(sc, cellx, celly, field, cond_mask=1, table_mask=1 << 4)


def test_one_cell_over_several_items_each_way_beside_narrow_ones(scene, tables):
    """A cell wider than two items' columns and taller than two items' rows, so that at least three items each way add
    to it, with cells of 25 pixels on either side; the sizes follow the library's item."""
    cols, rows = gpu.grid_rain_item()
    assert cols * rows <= 65535
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
    ncx, ncy = int(cellx.max()) + 1, int(celly.max()) + 1
    field = field_for(ncx, ncy)
    assert wide * tall > 4 * cols * rows                # more pixels than four items count
    got = check_rain(sc, cellx, celly, field, table_mask=0x81)
    assert got[0, big_y, big_x, 1] > 0


def test_sums_beyond_32_bits(scene):
    """A cell of 90 601 pixels of value 100 with the table "all 65535": sw passes 2^32."""
    t = np.full((9, 256, 5), 100, np.int32)
    W = H = 301
    inp = Inputs(W, H, 25, 5, t)
    inp.coarse[:] = 2                       # a valid soil everywhere: no pixel is 255
    inp.soil = inp.coarse[inp.cj[:, None], inp.ci[None, :]]
    sc = scene(inp)
    cellx, celly = np.zeros(W, np.int32), np.zeros(H, np.int32)
    w = np.stack([Q50, stormutil.POOL["all 65535"]])
    got = check_rain(sc, cellx, celly, np.full((1, 1), 1, np.uint8), w, table_mask=0x11)
    n = got[0, 0, 0, 1]
    assert n >= 90000 and got[0, 0, 0, 0] == 100 * n and got[0, 0, 0, 2] == 65535 * n > (1 << 32)


def test_one_single_pair_with_cell_edges_inside_a_wave_a_lane_and_on_a_group_boundary(scene, tables):
    """Constant landcover and soil, so that whole waves take the one-add path of count16; cell edges 16 k + 7 (inside a
    lane's 16 pixels), 16 k (between two lanes) and a cell that several waves span."""
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
    got = check_rain(sc, cellx, celly, field_for(5, 2))
    np.testing.assert_array_equal(got[0, :, :, 1], np.outer([9, 15], [80, 71, 1056, 9, 884]))


# ---- ADD semantics --------------------------------------------------------------------------------------------------

def test_two_calls_cut_inside_a_cell_row_add_up_to_one(scene, tables):
    sc = strip(scene, tables)
    cellx, celly = maps(W1, ROWS1, 100, 25.6, (5, 3), (3, 2))
    field = field_for(int(cellx.max()) + 1, int(celly.max()) + 1)
    whole = check_rain(sc, cellx, celly, field)
    cut = 31
    assert celly[cut - 1] == celly[cut] >= 0
    parts = check_rain(sc, cellx, celly, field, bands=[(0, cut), (cut, ROWS1 - cut)])
    np.testing.assert_array_equal(parts, whole)


def test_a_second_call_doubles_every_triple(scene, tables):
    sc = strip(scene, tables)
    cellx, celly = maps(W1, ROWS1, 17.3, 15.9, (5, 3), (3, 2))
    field = field_for(int(cellx.max()) + 1, int(celly.max()) + 1)
    once = check_rain(sc, cellx, celly, field)
    twice = run_rain(sc, cellx, celly, field, TABLES, repeat=2)
    np.testing.assert_array_equal(twice, 2 * once)
    assert once[..., 1].max() > 0 and once[..., 2].max() > 0


# ---- memory safety --------------------------------------------------------------------------------------------------

def test_maps_and_fields_that_break_the_rules_write_nothing_outside(scene, tables):
    """Map entries >= ncx, >= ncy, negative and INT_MIN count as "in no cell", field entries >= k as table 0; the
    guards around acc stay (run_rain asserts it), the landcover ends with its allocation, and the words are those of
    the valid entries."""
    sc = strip(scene, tables)
    cellx, celly = maps(W1, ROWS1, 8, 8, (5, 3), (3, 2))
    ncx, ncy = int(cellx.max()) + 1 - 3, int(celly.max()) + 1 - 1      # the last cells are beyond acc
    rng = np.random.default_rng(8)
    cellx, celly = cellx.copy(), celly.copy()
    for m, n in ((cellx, ncx), (celly, ncy)):
        at = rng.permutation(len(m))[:len(m) // 6]
        m[at] = rng.choice([INT_MIN, -7, n, n + 5, 2 ** 31 - 1, -1], len(at))
    k = 7
    field = field_for(ncx, ncy)
    assert (field >= k).any() and (cellx >= ncx).any() and (celly >= ncy).any() and (cellx == INT_MIN).any()
    check_rain(sc, cellx, celly, field, TABLES[:k])
    # maps whose entries decrease: unspecified sums by the contract, memory-safe; this kernel sums them all the same
    check_rain(sc, cellx[::-1].copy(), celly[::-1].copy(), field, TABLES[:k], table_mask=0x3)


# ---- grid_finish_rain -----------------------------------------------------------------------------------------------

def test_finish_on_hand_made_triples(engine, tables):
    """Every branch of the cell rule against a rising table (bisection) and one that decreases (the scan), n = 0,
    sw = 0, and triples no c reaches; shared cells packed with n_shared > 0 and = 0."""
    engine.set_tables(tables)
    down = Q50.copy()
    down[40:60] = down[40:60][::-1]
    three = np.stack([Q50, down, stormutil.POOL["random"]])
    triples = hand_made_triples(Q50) + [(50, 1, 65536), (50 << 20, 1 << 20, 65535 << 21), (7, 1, 1 << 40)]
    n = len(triples)
    field = (np.arange(n) % 5).astype(np.uint8)             # 3 and 4 name no table: table 0
    acc = np.array([triples, triples[::-1]], np.int64)
    idx = [0, n - 1, 3, 3, 0]
    means, cnq, shared = run_finish_rain(engine, acc, field, three, idx)
    want = rn.cn_cells(acc, field, three)
    np.testing.assert_array_equal(cnq, want)
    assert [host.runoff_cn(*tr, three[rn.clamp_field(field, 3)[c]]) for c, tr in enumerate(triples)] == want[0].tolist()
    np.testing.assert_array_equal(means, rn.means(acc))
    np.testing.assert_array_equal(shared, acc[:, idx, :])
    assert (cnq[0][:2] == 255).all() and 100 in cnq[0][-3:]
    means, cnq, shared = run_finish_rain(engine, acc, field, three, [])    # n_shared = 0: no pointer is touched
    np.testing.assert_array_equal(cnq, want)
    assert shared.shape == (2, 0, 3)


def test_finish_on_the_sums_of_a_scene(scene, tables):
    sc = strip(scene, tables)
    cellx, celly = maps(W1, ROWS1, 25, 25.6, (5, 3), (3, 2))
    ncx, ncy = int(cellx.max()) + 1, int(celly.max()) + 1
    field = field_for(ncx, ncy)
    field[0, :4] = (0, 3, 7, 255)           # no rain, a table that decreases, and the largest depth
    acc = check_rain(sc, cellx, celly, field).reshape(18, -1, 3)
    idx = [0, ncx * ncy - 1, 7, 7]
    means, cnq, shared = run_finish_rain(sc.eng, acc, field, TABLES, idx)
    np.testing.assert_array_equal(means, rn.means(acc))
    np.testing.assert_array_equal(cnq, rn.cn_cells(acc, field, TABLES))
    np.testing.assert_array_equal(shared, acc[:, idx, :])
    np.testing.assert_array_equal(cnq[:, 0], means[:, 0])       # byte 0: the table is all zero, sw = 0, the mean byte
    assert (acc[:, 0, 2] == 0).all() and (acc[:, 3, 2] > 0).any()


# ---- state and errors -----------------------------------------------------------------------------------------------

def _sums(eng, esa, cj, cx, cy, field, acc, W=32, rows=4, ncx=2, ncy=1, cond=3, table=0x1FF):
    rc = gpu.lib().gcn10_gpu_grid_sums_rain(eng._ctx, esa, W, rows, cj, cx, cy, ncx, ncy, cond, table, field, acc, None)
    return rc, gpu.lib().gcn10_gpu_last_error().decode()


def test_state_and_errors(tables):
    eng = gpu.Engine(0)
    L = gpu.lib()
    try:
        inp = Inputs(32, 4, 8, 3, tables)
        cellx, celly = (np.arange(32) // 16).astype(np.int32), np.zeros(4, np.int32)
        field = np.array([1, 9], np.uint8)                  # 9 names no table: table 0
        bufs = [eng.upload(a) for a in (inp.esa, inp.coarse, inp.ci, inp.cj, cellx, celly, field)]
        nbytes = 18 * 2 * 24
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
        rc = L.gcn10_gpu_grid_finish_rain(eng._ctx, acc.ptr, 18, 2, fld, o, o + 64, None, 0, None, None)
        assert rc == E_STATE and "gcn10_gpu_set_rain_tables" in L.gcn10_gpu_last_error().decode()
        for w, k in ((None, 1), (two.ctypes.data, 0), (two.ctypes.data, -1), (two.ctypes.data, 257)):
            rc = L.gcn10_gpu_set_rain_tables(eng._ctx, w, k)
            assert rc == E_INVAL and "gcn10_gpu_set_rain_tables" in L.gcn10_gpu_last_error().decode(), (w, k)
        eng.set_weights(Q50)                # independent of the weighted calls' tables, either way round
        eng.set_rain_tables(two)
        eng.set_weight_tables(two)
        eng.set_tables(tables)              # voids the weights, not the rain tables
        rc, msg = _sums(eng, esa, cj, cx, cy, fld, acc.ptr, W=48)
        assert rc == E_STATE and "prepare" in msg, (rc, msg)
        bad = [dict(rows=0), dict(rows=-1), dict(ncx=0), dict(ncx=-2), dict(ncy=0), dict(ncy=-1), dict(cond=0),
               dict(cond=4), dict(table=0), dict(table=1 << 9), dict(cx=None), dict(cy=None), dict(field=None),
               dict(acc=None)]
        for kw in bad:
            args = dict(cx=cx, cy=cy, field=fld, acc=acc.ptr)
            args.update(kw)
            rc, msg = _sums(eng, esa, cj, **args)
            assert rc == E_INVAL and "gcn10_gpu_grid_sums_rain" in msg, (kw, rc, msg)
        for args in ((acc.ptr, 0, 2, fld, o, o + 64, None, 0, None), (acc.ptr, 19, 2, fld, o, o + 64, None, 0, None),
                     (acc.ptr, 18, 0, fld, o, o + 64, None, 0, None), (None, 18, 2, fld, o, o + 64, None, 0, None),
                     (acc.ptr, 18, 2, None, o, o + 64, None, 0, None), (acc.ptr, 18, 2, fld, None, o + 64, None, 0, None),
                     (acc.ptr, 18, 2, fld, o, None, None, 0, None), (acc.ptr, 18, 2, fld, o, o + 64, None, 1, acc.ptr),
                     (acc.ptr, 18, 2, fld, o, o + 64, cx, 1, None)):
            rc = L.gcn10_gpu_grid_finish_rain(eng._ctx, *args, None)
            assert rc == E_INVAL and "gcn10_gpu_grid_finish_rain" in L.gcn10_gpu_last_error().decode(), args
        eng.sync()
        assert (eng.download(acc.ptr, (nbytes,)) == POISON).all(), "a refused call wrote"
        assert (eng.download(out.ptr, (256,)) == POISON).all(), "a refused call wrote"
        # and the good call, after all that: the rain tables outlived set_tables
        eng.memset(acc.ptr, 0, nbytes)
        rc, msg = _sums(eng, esa, cj, cx, cy, fld, acc.ptr)
        assert rc == OK, msg
        eng.sync()
        got = eng.download(acc.ptr, (nbytes,)).view(np.uint64).astype(np.int64).reshape(18, 1, 2, 3)
        want = np.zeros((18, 1, 2, 3), np.int64)
        for r in range(18):
            rn.add_triples(want[r], au.oracle_rasters(inp.esa, inp.soil, tables, [r])[r], cellx, celly,
                           field.reshape(1, 2), two)
        np.testing.assert_array_equal(got, want)
        cols, rows = gpu.grid_rain_item()
        assert cols % 16 == 0 and 0 < cols * rows <= 65535
    finally:
        eng.sync()
        eng.close()
