"""GPU: area means on a coarser grid (gcn10_gpu_aggregate) through the ABI face.  Needs an MI355X.

Expected values: the oracle's full-resolution rasters (modify_hysogs_data + calculate_cn over coarse[cj][:, ci], as
tests/test_gpu_soil_tables.py takes them) reduced in numpy by the definition (tests/aggutil.py).  Every comparison is
bit-exact.  Shapes are the smallest at which the kernels can go wrong: factors on both sides of the 16-pixel column
group (the kernel for f < 16 and the one for f >= 16), widths around a group and around the 4080 columns of a
workgroup's chunk, first and last columns inside a group, a clipped last cell and last cell row, rows < f.
"""
import ctypes as C

import numpy as np
import pytest

from gcn10_amd import gpu, host
from tests import aggutil as au
from tests.util import ESA_NASTY, HSG_NASTY, random_tables

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_STATE = 0, -1, -4
POISON = 0xA5
GUARD = 64
FACTORS = [2, 3, 15, 16, 17, 25, 100, 256]
WIDTHS = [1, 15, 16, 17, 1039, 1040, 1041, 2064]
_SCENES = {}            # key -> the host side of a scene (inputs and the oracle's rasters), made once and shared


def x_ranges(W):
    return [(a, b) for a, b in ((0, W), (1, W), (0, W - 1), (5, W - 3)) if 0 <= a < b]


class Inputs:
    """Landcover in patches with noise, a soil window at `ratio` columns per cell, index maps whose cj repeats and
    goes back (as in tests/test_gpu_zonal.py), and the oracle's rasters for `tables`."""

    def __init__(self, W, rows, ratio, seed, tables):
        rng = np.random.default_rng(seed)
        self.W, self.rows, self.tables = W, rows, tables
        small = rng.choice(ESA_NASTY, size=((rows + 5) // 6, (W + 8) // 9))
        esa = np.repeat(np.repeat(small, 6, axis=0), 9, axis=1)[:rows, :W]
        noise = rng.integers(0, 256, size=esa.shape)
        self.esa = np.ascontiguousarray(np.where(noise < 60, rng.choice(ESA_NASTY, size=esa.shape), esa).astype(np.uint8))
        self.hsx, self.hsy = int(W / ratio) + 2, int(rows / ratio) + 3
        self.coarse = rng.choice(HSG_NASTY, size=(self.hsy, self.hsx)).astype(np.uint8)
        gt = [0.0, 1.0 / W, 0.0, 1.0, 0.0, -1.0 / W]
        sgt = [-0.013 * ratio / W, ratio / W, 0.0, 1.0 + 0.02 * ratio / W, 0.0, -ratio / W]
        ci, cj = host.build_index_maps(gt, sgt, W, rows, self.hsx, self.hsy)
        cj = cj.copy()
        cj[rows // 2:] = cj[rows // 2:][::-1]               # decreasing
        cj[rows // 4:rows // 4 + 3] = cj[rows // 4]         # repeated
        self.ci, self.cj = ci, cj
        self.soil = self.coarse[cj[:, None], ci[None, :]]
        self._want = {}

    def want(self, r):
        if r not in self._want:
            self._want.update(au.oracle_rasters(self.esa, self.soil, self.tables, [r]))
        return self._want[r]


def inputs(key, W, rows, ratio, seed, tables):
    if key not in _SCENES:
        _SCENES[key] = Inputs(W, rows, ratio, seed, tables)
    return _SCENES[key]


class Scene:
    """Inputs on the device (landcover `offset` bytes into its allocation), tile prepared."""

    def __init__(self, eng, inp, offset=1):
        self.eng, self.inp = eng, inp
        eng.set_tables(inp.tables)
        self.esa_buf = eng.alloc(inp.esa.nbytes + offset)
        self.esa_ptr = self.esa_buf.ptr + offset
        eng.h2d(self.esa_ptr, inp.esa)
        self.bufs = [self.esa_buf] + [eng.upload(a) for a in (inp.coarse, inp.ci, inp.cj)]
        eng.prepare_tile(self.bufs[1].ptr, inp.hsx, inp.hsy, self.bufs[2].ptr, inp.W)

    def run(self, x0, x1, f, cond_mask=3, table_mask=0x1FF, band=None, extra=7, rows=None):
        """{r: uint8[Ha][Wa]} of the selected rasters; asserts that no byte outside the cells was written."""
        inp, eng = self.inp, self.eng
        rows = inp.rows if rows is None else rows
        sel = au.selected(cond_mask, table_mask)
        Wa, Ha = au.cells(x1 - x0, f), au.cells(rows, f)
        stride = Wa + extra
        slot = Ha * stride + GUARD
        out = eng.alloc(len(sel) * slot)
        try:
            eng.memset(out.ptr, POISON, len(sel) * slot)
            step = band or rows
            assert step % f == 0 or step >= rows
            for y0 in range(0, rows, step):
                n = min(step, rows - y0)
                ptrs = [out.ptr + q * slot + (y0 // f) * stride for q in range(len(sel))]
                eng.aggregate(self.esa_ptr + y0 * inp.W, inp.W, n, self.bufs[3].ptr + 4 * y0, x0, x1, f, cond_mask,
                              table_mask, ptrs, stride)
            eng.sync()
            img = eng.download(out.ptr, (len(sel), slot))
        finally:
            eng.sync()
            out.close()
        got = {}
        for q, r in enumerate(sel):
            body = img[q, :Ha * stride].reshape(Ha, stride)
            assert (body[:, Wa:] == POISON).all(), "raster %d: bytes between the rows were written" % r
            assert (img[q, Ha * stride:] == POISON).all(), "raster %d: bytes behind the last row were written" % r
            got[r] = body[:, :Wa]
        return got

    def check(self, x0, x1, f, cond_mask=3, table_mask=0x1FF, band=None, rows=None):
        got = self.run(x0, x1, f, cond_mask, table_mask, band=band, rows=rows)
        rows = self.inp.rows if rows is None else rows
        for r, g in got.items():
            want = au.reduce_raster(self.inp.want(r)[:rows], x0, x1, f)
            bad = np.argwhere(g != want)
            assert bad.size == 0, "W=%d rows=%d [%d, %d) f=%d raster %d: %d cells differ, first (cy, cx) = %s: got %d, " \
                "want %d" % (self.inp.W, rows, x0, x1, f, r, len(bad), tuple(bad[0]), g[tuple(bad[0])], want[tuple(bad[0])])
        return got

    def close(self):
        self.eng.sync()
        for b in self.bufs:
            b.close()


@pytest.fixture
def scene(engine):
    made = []

    def make(inp, offset=1):
        made.append(Scene(engine, inp, offset))
        return made[-1]
    yield make
    for s in made:
        s.close()
    engine.set_option("defaults", 0)


def reference_paths(inp, x0, x1, f, rasters=range(18)):
    """(cells that are 255 because n = 0, cells with 0 < n < footprint, exact ties that round up) over the rasters."""
    empty = partial = ties = 0
    for r in rasters:
        s, n, area = au.reduce_sums(inp.want(r), x0, x1, f)
        empty += int((n == 0).sum())
        partial += int(((n > 0) & (n < area)).sum())
        ties += int(((n > 0) & ((2 * s + n) % (2 * np.maximum(n, 1)) == 0)).sum())
    return empty, partial, ties


# ---- factors, widths, column ranges ------------------------------------------------------------------------------

@pytest.mark.parametrize("f", FACTORS)
def test_every_factor_equals_the_reduced_oracle(scene, tables, f):
    """1041 x 230: three cell rows at f = 100 (the last of 30 rows), rows < f at 256, clipped last cells everywhere."""
    inp = inputs("factors", 1041, 230, 25, 11, tables)
    sc = scene(inp)
    for x0, x1 in x_ranges(inp.W):
        sc.check(x0, x1, f)


def test_the_reference_reaches_empty_cells_partial_cells_and_ties(tables):
    """The paths the comparison above is about are in its reference (no GPU work: the oracle and numpy alone)."""
    inp = inputs("factors", 1041, 230, 25, 11, tables)
    for f in (2, 3, 16, 25):
        empty, partial, ties = reference_paths(inp, 5, inp.W - 3, f)
        assert empty > 0 and partial > 0 and ties > 0, (f, empty, partial, ties)


@pytest.mark.parametrize("f", [3, 25])
@pytest.mark.parametrize("W", WIDTHS)
def test_widths_around_the_column_group(scene, tables, W, f):
    inp = inputs(("width", W), W, 60, 25, 20 + W, tables)
    sc = scene(inp)
    for x0, x1 in x_ranges(W):
        sc.check(x0, x1, f)


def test_one_cell_when_the_factor_exceeds_width_and_rows(scene, tables):
    inp = inputs(("width", 17), 17, 60, 25, 20 + 17, tables)
    sc = scene(inp)
    for f in (61, 256):
        got = sc.check(0, 17, f)
        assert got[0].shape == (1, 1)
    got = sc.check(5, 14, 16, rows=9)           # rows < f
    assert got[0].shape == (1, 1)


@pytest.mark.parametrize("offset", [0, 1, 3])
def test_landcover_at_any_byte_offset(scene, tables, offset):
    inp = inputs(("width", 1041), 1041, 60, 25, 20 + 1041, tables)
    sc = scene(inp, offset=offset)
    sc.check(5, 1038, 25)
    sc.check(5, 1038, 7)


# ---- soil ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ratio, state", [(25.3, 1), (16, 1), (10.2, 2)])
def test_soil_cells_of_25_16_and_10_columns(scene, tables, ratio, state):
    """About 10 columns per soil cell put three cells under a 16-pixel group: a complex tile."""
    inp = inputs(("soil", ratio), 1040, 120, ratio, 31, tables)
    sc = scene(inp, offset=0)
    assert sc.eng.soil_words_state() == state
    for f in (25, 16, 5):
        sc.check(0, 1040, f)
        sc.check(3, 1033, f)


@pytest.mark.parametrize("n_tables", [9, 5])
def test_awkward_tables_and_mask_subsets(scene, n_tables):
    t = random_tables(5, n_tables)
    inp = inputs(("nasty", n_tables), 333, 77, 25, 41, t)
    sc = scene(inp)
    full = (1 << n_tables) - 1
    empty, partial, ties = reference_paths(inp, 1, 333, 3, range(n_tables))
    assert empty > 0 and partial > 0 and ties > 0
    for cond_mask in (1, 2, 3):
        for table_mask in (full, 1, 1 << (n_tables - 1), 0x15 & full):
            for f in (3, 25):
                got = sc.check(1, 333, f, cond_mask, table_mask)
                assert sorted(got) == au.selected(cond_mask, table_mask)


def test_hand_made_footprints(scene):
    """f = 2; classes 10 and 20 give 10 and 11 on every soil, everything else 255."""
    t = np.full((1, 256, 5), 255, np.int32)
    t[0, 10, :], t[0, 20, :] = 10, 11
    inp = Inputs(6, 2, 25, 1, t)
    inp.esa = np.array([[10, 20, 10, 10, 30, 30], [30, 30, 20, 30, 30, 30]], np.uint8)
    inp.coarse[:] = 1
    inp.soil = inp.coarse[inp.cj[:, None], inp.ci[None, :]]
    sc = scene(inp)
    got = sc.check(0, 6, 2, 1, 1)
    assert got[0].tolist() == [[11, 10, 255]]


# ---- bands --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("f", [3, 25])
def test_bands_give_the_bytes_of_one_call(scene, tables, f):
    inp = inputs("factors", 1041, 230, 25, 11, tables)
    sc = scene(inp)
    whole = sc.check(5, 1038, f)
    for band in (f, 3 * f):
        got = sc.run(5, 1038, f, band=band)
        for r in whole:
            np.testing.assert_array_equal(got[r], whole[r], err_msg="bands of %d rows, raster %d" % (band, r))


def test_a_row_of_a_real_block(scene, tables):
    """36001 columns of which 36000 are owned: nine chunks per cell row, the last one clipped."""
    inp = inputs("wide", 36001, 75, 25, 51, tables)
    sc = scene(inp)
    got = sc.check(0, 36000, 25)
    assert got[0].shape == (3, 1440)


def test_factor_2_equals_level_1_of_the_average_overviews(scene, tables):
    """A cross-check between two GPU paths, not the parity claim (that is the oracle's, above)."""
    inp = inputs("overview", 301, 512, 25, 61, tables)
    sc = scene(inp, offset=0)
    eng = sc.eng
    got = sc.check(0, 301, 2)
    h, w = 256, 151
    out = eng.alloc(18 * h * w)
    try:
        ptrs = [out.ptr + r * h * w for r in range(18)]
        for y0 in (0, 256):
            eng.overview_average(sc.esa_ptr, 301, 512, y0, 256, sc.bufs[3].ptr, 3, 0x1FF, 1, ptrs)
        eng.sync()
        level1 = eng.download(out.ptr, (18, h, w))
    finally:
        eng.sync()
        out.close()
    for r in range(18):
        np.testing.assert_array_equal(got[r], level1[r], err_msg="raster %d" % r)


# ---- errors -------------------------------------------------------------------------------------------------------

def _call(eng, esa, cj, out, W=32, rows=4, x0=0, x1=32, f=2, cond=3, table=0x1FF, stride=64):
    ptrs = (C.c_void_p * 18)(*[out.ptr + r * 1024 for r in range(18)])
    rc = gpu.lib().gcn10_gpu_aggregate(eng._ctx, esa, W, rows, cj, x0, x1, f, cond, table, ptrs, stride, None)
    return rc, gpu.lib().gcn10_gpu_last_error().decode()


def test_errors(tables):
    eng = gpu.Engine(0)
    try:
        inp = Inputs(32, 4, 8, 3, tables)
        bufs = [eng.upload(a) for a in (inp.esa, inp.coarse, inp.ci, inp.cj)]
        out = eng.alloc(18 * 1024)
        eng.memset(out.ptr, POISON, 18 * 1024)
        esa, cj = bufs[0].ptr, bufs[3].ptr
        rc, msg = _call(eng, esa, cj, out)
        assert rc == E_STATE and "gcn10_gpu_set_tables" in msg, (rc, msg)
        eng.set_tables(tables)
        rc, msg = _call(eng, esa, cj, out)
        assert rc == E_STATE and "prepare" in msg, (rc, msg)
        eng.prepare_tile(bufs[1].ptr, inp.hsx, inp.hsy, bufs[2].ptr, 32)
        rc, msg = _call(eng, esa, cj, out, W=48, x1=48)
        assert rc == E_STATE and "prepare" in msg, (rc, msg)
        bad = [dict(f=1), dict(f=0), dict(f=257), dict(x0=-1), dict(x0=32), dict(x0=7, x1=7), dict(x1=33), dict(rows=0),
               dict(rows=-1), dict(stride=15), dict(cond=0), dict(cond=4), dict(table=0), dict(table=1 << 9)]
        for kw in bad:
            rc, msg = _call(eng, esa, cj, out, **kw)
            assert rc == E_INVAL and "gcn10_gpu_aggregate" in msg, (kw, rc, msg)
        eng.sync()
        assert (eng.download(out.ptr, (18 * 1024,)) == POISON).all(), "a refused call wrote"
        rc, msg = _call(eng, esa, cj, out, stride=16)        # the smallest stride there is
        assert rc == OK, msg
        eng.sync()
        got = eng.download(out.ptr, (18, 1024))
        for r in range(18):
            want = au.reduce_raster(au.oracle_rasters(inp.esa, inp.soil, tables, [r])[r], 0, 32, 2)
            np.testing.assert_array_equal(got[r, :32].reshape(2, 16), want)
            assert (got[r, 32:] == POISON).all()
    finally:
        eng.sync()
        eng.close()
