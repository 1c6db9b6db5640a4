"""GPU: gcn10_gpu_runoff_strip, the rasters of a strip through a byte table per cell of a coarse grid, and
gcn10_gpu_set_cell_byte_tables.  Needs an MI355X.

Expected values: T[table of the pixel's cell][value of the oracle's raster], composed in numpy (want_raster) -- never
another GPU path.  Every output lies between guard bytes in a poisoned buffer.

Shapes: W in {5, 17, 300} takes the pixel path, 1040 is the narrowest strip of the 16-pixel lanes, 1043 / 2051 have a lane
that straddles a row end, 2048 has none, 36001 x 8 has a W * rows % 16 tail behind 35 waves of a row.
"""
import numpy as np
import pytest

from gcn10_amd import gpu
from tests import soil_readers as sr
from tests.test_gpu_soil_tables import eng9  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_STATE = 0, -1, -4
POISON, GUARD = 0xA5, 256
SHAPES = [(5, 40), (17, 40), (300, 40), (1040, 40), (1043, 40), (2048, 40), (2051, 40), (36001, 8)]
ALL = (3, 0x1FF)


def random_tables(k, seed=7):
    """k tables of random bytes: nothing leans on runoff's monotonicity, and T[t][255] is whatever it is"""
    return np.random.default_rng(seed + k).integers(0, 256, (k, 256)).astype(np.uint8)


def cell_map(kind, n):
    """(map int32[n], number of cells): the pixel -> cell maps of the tests, for columns or rows"""
    x = np.arange(n)
    if kind in ("1", "3", "16", "37.3"):
        m = np.floor(x / float(kind)).astype(np.int64)
        return m.astype(np.int32), int(m.max()) + 1
    if kind == "one":                           # one cell larger than the strip
        return np.zeros(n, np.int32), 1
    if kind == "edges":                         # -1 runs at both ends and scattered, entries >= the number of cells
        m = np.floor(x / 37.3).astype(np.int64)
        nc = int(m.max()) + 1
        lead, trail = min(21, n // 4), min(19, n // 4)
        m[:lead] = -1
        m[n - trail:] = -1
        at = np.random.default_rng(n).choice(n, size=max(2, n // 20), replace=False)
        m[at] = np.array([-1, nc, nc + 7, 2 ** 31 - 1, -2 ** 31, -5])[np.arange(at.size) % 6]
        return m.astype(np.int32), nc
    if kind == "decreasing":
        m = np.floor(x / 37.3).astype(np.int64)
        return (m.max() - m).astype(np.int32), int(m.max()) + 1
    if kind == "repeating":                     # three cells, each named by many runs
        return ((x // 16) % 3).astype(np.int32), 3
    if kind == "none":
        return np.full(n, -1, np.int32), 1
    raise KeyError(kind)


def want_raster(v, cellx, celly, ncx, ncy, field, T):
    """The contract in numpy: v = the oracle's raster (H x W), field = cell_table [ncy][ncx], T = [k][256]"""
    okx, oky = (cellx >= 0) & (cellx < ncx), (celly >= 0) & (celly < ncy)
    t = field[np.where(oky, celly, 0)][:, np.where(okx, cellx, 0)].astype(np.int64)
    t = np.where(t < len(T), t, 0)
    out = T[t, v]
    out[~(oky[:, None] & okx[None, :])] = 255
    return out


def tile_for(eng, tables, W, H, offsets=None):
    hsx, hsy = max(1, min(90, W // 3)), 6 if H >= 12 else 2
    return sr.ReaderTile(eng, tables, 500 + W, W, H, hsx, hsy, key="runoff-%dx%d" % (W, H), offsets=offsets)


class Run:
    """One tile, one pair of maps, one field and one set of tables: the calls over `strips` into poisoned rasters."""

    def __init__(self, t, xkind, ykind, k, masks=ALL, out_offset=0, field=None, T=None, set_tables=True):
        self.t, self.eng, self.masks, self.off = t, t.eng, masks, out_offset
        self.cellx, self.ncx = cell_map(xkind, t.W)
        self.celly, self.ncy = cell_map(ykind, t.H)
        self.T = random_tables(k) if T is None else T
        self.field = (np.random.default_rng(t.W + k).integers(0, 256, (self.ncy, self.ncx)).astype(np.uint8)
                      if field is None else field)
        self.sel = sr.selected(*masks)
        self.n = t.W * t.H
        self.slot = (GUARD + self.n + 3 + GUARD + 255) & ~255
        self.bufs = [self.eng.upload(a) for a in (self.cellx, self.celly, self.field)]
        self.out = self.eng.alloc(18 * self.slot)
        self.bufs.append(self.out)
        if set_tables:
            self.eng.set_cell_byte_tables(self.T)

    def ptr(self, r, y0=0):
        return self.out.at(r * self.slot + GUARD + self.off + y0 * self.t.W)

    def launch(self, strips=None, stream=None, unselected=None):
        t = self.t
        self.eng.memset(self.out.ptr, POISON, 18 * self.slot, stream)
        for y0, rows in strips or [(0, t.H)]:
            ptrs = [self.ptr(r, y0) if r in self.sel else unselected for r in range(18)]
            self.eng.runoff_strip(t.bufs[0].at(y0 * t.W), t.W, rows, t.bufs[3].at(4 * y0), self.bufs[0].ptr,
                                  self.bufs[1].at(4 * y0), self.ncx, self.ncy, self.bufs[2].ptr, self.masks[0],
                                  self.masks[1], ptrs, stream)

    def want(self, r):
        return want_raster(self.t.want(r), self.cellx, self.celly, self.ncx, self.ncy, self.field, self.T)

    def check(self, what=""):
        t = self.t
        self.eng.sync()
        img = self.eng.download(self.out.ptr, (18, self.slot))
        a = GUARD + self.off
        for r in range(18):
            if r not in self.sel:
                assert (img[r] == POISON).all(), "%s: raster %d is not selected and was written" % (what, r)
                continue
            got, want = img[r, a:a + self.n].reshape(t.H, t.W), self.want(r)
            bad = np.argwhere(got != want)
            assert bad.size == 0, "%s W=%d: raster %d differs in %d pixels, first at (y, x) = %s: got %d, want %d" % (
                what, t.W, r, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
            assert (img[r, :a] == POISON).all() and (img[r, a + self.n:] == POISON).all(), \
                "%s W=%d: raster %d was written outside its %d pixels" % (what, t.W, r, self.n)
        return img

    def close(self):
        for b in self.bufs:
            b.close()


def run_case(eng, tables, W, H, xkind, ykind, k, strips=None, **kw):
    t = tile_for(eng, tables, W, H, offsets=kw.pop("offsets", None))
    rn = None
    try:
        t.prepare()
        rn = Run(t, xkind, ykind, k, **kw)
        rn.launch(strips)
        rn.check("%s x %s, k=%d" % (xkind, ykind, k))
    finally:
        eng.sync()
        if rn is not None:
            rn.close()
        t.close()


@pytest.mark.parametrize("W,H", SHAPES)
def test_widths(eng9, tables, W, H):
    """every width: cells of 37.3 px with -1 runs, scattered -1 and entries >= ncx across, cells of 3 rows down, 256
    random tables, all 18 rasters"""
    run_case(eng9, tables, W, H, "edges", "3", 256)


@pytest.mark.parametrize("W", [300, 2051])
@pytest.mark.parametrize("xkind,ykind", [("1", "1"), ("3", "3"), ("16", "16"), ("37.3", "37.3"), ("one", "one"),
                                         ("edges", "edges"), ("decreasing", "decreasing"), ("repeating", "repeating"),
                                         ("37.3", "none")])
def test_maps(eng9, tables, W, xkind, ykind):
    run_case(eng9, tables, W, 40, xkind, ykind, 256)


def test_celly_all_outside_is_255_everywhere(eng9, tables):
    t = tile_for(eng9, tables, 2051, 40)
    try:
        t.prepare()
        rn = Run(t, "37.3", "none", 2)
        rn.launch()
        img = rn.check("no cell row")
        assert (img[:, GUARD:GUARD + rn.n] == 255).all()
        rn.close()
    finally:
        eng9.sync()
        t.close()


@pytest.mark.parametrize("W", [300, 1043, 2048])
@pytest.mark.parametrize("k", [1, 2, 256])
def test_table_counts(eng9, tables, W, k):
    """k random tables under a field of all 256 bytes: an entry >= k reads table 0"""
    run_case(eng9, tables, W, 40, "16", "3", k)


@pytest.mark.parametrize("W", [300, 2051])
def test_identity_tables_reproduce_cn_strip(eng9, tables, W):
    t = tile_for(eng9, tables, W, 40)
    try:
        t.prepare()
        rn = Run(t, "one", "one", 3, T=np.tile(np.arange(256, dtype=np.uint8), (3, 1)))
        rn.launch()
        img = rn.check("identity")
        for r in range(18):
            np.testing.assert_array_equal(img[r, GUARD:GUARD + rn.n].reshape(40, W), t.want(r))
        rn.close()
    finally:
        eng9.sync()
        t.close()


@pytest.mark.parametrize("W", [300, 2051])
def test_table_entry_255_is_applied_as_given(eng9, tables, W):
    T = random_tables(4)
    T[:, 255] = (7, 0, 254, 9)
    t = tile_for(eng9, tables, W, 40)
    try:
        t.prepare()
        rn = Run(t, "37.3", "3", 4, T=T)
        rn.launch()
        rn.check("T[t][255] != 255")
        assert any((t.want(r) == 255).any() for r in range(18)), "the tile has no pixel without a value"
        rn.close()
    finally:
        eng9.sync()
        t.close()


@pytest.mark.parametrize("W", [300, 2048, 2051])
@pytest.mark.parametrize("masks", [(1, 1 << 4), (2, 0x1FF), (3, 0x0A1)], ids=["one raster", "one condition", "three tables"])
def test_raster_subsets(eng9, tables, W, masks):
    """unselected entries of out[] are NULL"""
    run_case(eng9, tables, W, 40, "edges", "3", 256, masks=masks)


@pytest.mark.parametrize("W", [300, 2048, 2051])
@pytest.mark.parametrize("esa_off,out_off", [(1, 0), (0, 3), (3, 1)])
def test_alignment(eng9, tables, W, esa_off, out_off):
    run_case(eng9, tables, W, 40, "edges", "3", 256, offsets=(esa_off, 0, 0, 0), out_offset=out_off)


@pytest.mark.parametrize("W", [300, 1043, 2048])
def test_three_calls_equal_one(eng9, tables, W):
    """strips of 13, 14 and 13 rows: they start inside a soil row, inside a cell row, and (W = 1043) off 16 bytes"""
    run_case(eng9, tables, W, 40, "edges", "edges", 256, strips=[(0, 13), (13, 14), (27, 13)])


def test_unselected_pointers_are_ignored(eng9, tables):
    t = tile_for(eng9, tables, 2051, 40)
    try:
        t.prepare()
        rn = Run(t, "16", "3", 2, masks=(1, 1 << 2))
        rn.launch(unselected=1)         # an address nobody may touch
        rn.check("unselected = 1")
        rn.close()
    finally:
        eng9.sync()
        t.close()


# ---- stale state ------------------------------------------------------------------------------------------------------

def test_set_tables_keeps_the_byte_tables_and_a_smaller_k_takes_effect(eng9, tables):
    t = tile_for(eng9, tables, 2051, 40)
    try:
        big = Run(t, "16", "3", 256)
        eng9.set_tables(tables)                     # after set_cell_byte_tables: the byte tables stay
        t.prepare()
        big.launch()
        big.check("after set_tables")
        small = Run(t, "16", "3", 2, field=big.field)   # bytes 2..255 now read table 0
        small.launch()
        small.check("k = 2 after k = 256")
        assert (small.T[:2] != big.T[:2]).any()
        big.close()
        small.close()
    finally:
        eng9.sync()
        t.close()


def test_wider_then_narrower_strip_on_one_context(eng9, tables):
    """the workspace of the expanded tables grows with the call and is written anew by every call"""
    for W, ykind in ((1043, "3"), (2051, "1"), (1043, "16"), (300, "3")):
        run_case(eng9, tables, W, 40, "edges", ykind, 256)


# ---- state and errors -------------------------------------------------------------------------------------------------

def _strip(eng, esa, cj, cx, cy, field, outs, W=32, rows=4, ncx=2, ncy=1, cond=3, table=0x1FF):
    import ctypes as C
    arr = None
    if outs is not None:
        arr = (C.c_void_p * 18)(*outs)
    rc = gpu.lib().gcn10_gpu_runoff_strip(eng._ctx, esa, W, rows, cj, cx, cy, ncx, ncy, field, cond, table, arr, None)
    return rc, gpu.lib().gcn10_gpu_last_error().decode()


def test_state_and_errors(tables):
    eng = gpu.Engine(0)
    L = gpu.lib()
    t = sr.ReaderTile(eng, tables, 77, 32, 4, 8, 3)
    try:
        cellx, celly = (np.arange(32) // 16).astype(np.int32), np.zeros(4, np.int32)
        field = np.array([1, 9], np.uint8)                  # 9 names no table: table 0
        T = random_tables(2)
        bufs = [eng.upload(a) for a in (cellx, celly, field)]
        slot = 256
        out = eng.alloc(18 * slot)
        eng.memset(out.ptr, POISON, 18 * slot)
        esa, cj, cx, cy, fld = t.bufs[0].ptr, t.bufs[3].ptr, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr
        outs = [out.at(r * slot + 64) for r in range(18)]
        rc, msg = _strip(eng, esa, cj, cx, cy, fld, outs)
        assert rc == E_STATE and "gcn10_gpu_set_tables" in msg, (rc, msg)
        eng.set_tables(tables)
        rc, msg = _strip(eng, esa, cj, cx, cy, fld, outs)
        assert rc == E_STATE and "prepare" in msg, (rc, msg)
        t.prepare()
        rc, msg = _strip(eng, esa, cj, cx, cy, fld, outs)
        assert rc == E_STATE and "call gcn10_gpu_set_cell_byte_tables first" in msg, (rc, msg)
        for w, k in ((None, 1), (T.ctypes.data, 0), (T.ctypes.data, -1), (T.ctypes.data, 257)):
            rc = L.gcn10_gpu_set_cell_byte_tables(eng._ctx, w, k)
            assert rc == E_INVAL and "gcn10_gpu_set_cell_byte_tables" in L.gcn10_gpu_last_error().decode(), (w, k)
        rc, msg = _strip(eng, esa, cj, cx, cy, fld, outs)
        assert rc == E_STATE and "call gcn10_gpu_set_cell_byte_tables first" in msg, (rc, msg)
        eng.set_cell_byte_tables(T)
        rc, msg = _strip(eng, esa, cj, cx, cy, fld, outs, W=48)
        assert rc == E_STATE and "prepare" in msg, (rc, msg)
        missing = list(outs)
        missing[5] = None
        bad = [dict(W=0), dict(W=-3), dict(rows=0), dict(rows=-1), dict(ncx=0), dict(ncx=-2), dict(ncy=0), dict(ncy=-1),
               dict(cond=0), dict(cond=4), dict(table=0), dict(table=1 << 9), dict(cx=None), dict(cy=None),
               dict(field=None), dict(outs=None), dict(outs=missing), dict(esa=None), dict(cj=None)]
        for kw in bad:
            args = dict(esa=esa, cj=cj, cx=cx, cy=cy, field=fld, outs=outs)
            args.update(kw)
            rc, msg = _strip(eng, **args)
            assert rc == E_INVAL and "gcn10_gpu_runoff_strip" in msg, (kw, rc, msg)
        eng.sync()
        assert (eng.download(out.ptr, (18 * slot,)) == POISON).all(), "a refused call wrote"
        # and the good call, after all that
        rc, msg = _strip(eng, esa, cj, cx, cy, fld, outs)
        assert rc == OK, msg
        eng.sync()
        img = eng.download(out.ptr, (18, slot))
        for r in range(18):
            want = want_raster(t.want(r), cellx, celly, 2, 1, field.reshape(1, 2), T)
            np.testing.assert_array_equal(img[r, 64:64 + 128].reshape(4, 32), want)
            assert (img[r, :64] == POISON).all() and (img[r, 192:] == POISON).all()
        assert eng.last_kernel_name() == "runoff_strip_kernel<256>"
    finally:
        eng.sync()
        t.close()
        eng.close()
