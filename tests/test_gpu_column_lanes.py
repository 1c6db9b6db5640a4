"""GPU: the strips of 16-byte aligned rows keep every lane in one column group (gcn10::strip_lane_plan) and take the
soil from the codes table through the lane's column entry.  Needs an MI355X.

Every selected raster is compared byte for byte with the oracle (tests/soil_readers.ReaderTile: calculate_cn /
modify_hysogs_data over coarse[cj][:, ci], computed once per tile and shared), inside guard bytes that must stay
untouched -- never with another GPU path."""
import numpy as np
import pytest

from tests import soil_readers as sr
from tests.test_gpu_soil_tables import K1, _with_complex_group

pytestmark = pytest.mark.gpu

GUARD = sr.GUARD
POISON = 0xA5
SUBSET = 0x0A1      # three of the nine tables


@pytest.fixture
def eng9(engine, tables):
    engine.set_tables(tables)
    yield engine
    engine.set_option("defaults", 0)


def run_strip(t, cond_mask, table_mask, what, y0=0, rows=None, kernel="cn_strip_kernel<"):
    """One cn_strip over rows [y0, y0 + rows) of the tile into rasters with guard bytes on both sides; every selected
    raster against the oracle, every guard byte untouched."""
    eng, W = t.eng, t.W
    rows = t.H - y0 if rows is None else rows
    n = W * rows
    sel = sr.selected(cond_mask, table_mask)
    slot = (n + 2 * GUARD + 255) & ~255
    arena = eng.alloc(len(sel) * slot)
    try:
        eng.memset(arena.ptr, POISON, len(sel) * slot)
        ptrs = [None] * 18
        for i, r in enumerate(sel):
            ptrs[r] = arena.at(i * slot + GUARD)
        eng.cn_strip(t.bufs[0].at(y0 * W), W, rows, t.bufs[3].at(4 * y0), cond_mask, table_mask, ptrs)
        name = eng.last_kernel_name()
        img = eng.download(arena.ptr, (len(sel), slot))
    finally:
        eng.sync()
        arena.close()
    assert name.startswith(kernel), "%s: ran %s" % (what, name)
    for i, r in enumerate(sel):
        got = img[i, GUARD:GUARD + n].reshape(rows, W)
        bad = np.argwhere(got != t.want(r)[y0:y0 + rows])
        assert bad.size == 0, "%s (%s): raster %d differs in %d pixels, first at (row, column) %s" % (
            what, name, r, len(bad), tuple(bad[0]))
        assert (img[i, :GUARD] == POISON).all() and (img[i, GUARD + n:] == POISON).all(), \
            "%s (%s): raster %d wrote outside its pixels" % (what, name, r)
    return name


def tile(eng, tables, key, **kw):
    return sr.ReaderTile(eng, tables, key="lanes-" + key, **kw)


# ---- a row end in every wave, several trips per piece with a ragged last one -------------------------------------

def _wide_ci(W, hsx, complex_tile):
    return _with_complex_group(W, hsx, 7) if complex_tile else None


@pytest.mark.parametrize("complex_tile", [False, True], ids=["compact", "complex"])
@pytest.mark.parametrize("what", ["one-table", "all-tables", "three-tables"])
@pytest.mark.parametrize("W", [1040, 1056])
def test_row_ends_in_every_wave(eng9, tables, W, what, complex_tile):
    """W = 1040 and 1056 (65 and 66 column groups: a row end inside every wave), 3100 rows on one workgroup per CU:
    at one sub-trip per trip every XCD's 387 or 388 rows take three full trips of 120 rows and a ragged one; at four
    sub-trips the grid (197 workgroups) is no multiple of 8 and the strip is one piece.  Both drainage conditions,
    every chunk count with and without the software pipeline; the complex tile goes pixel by pixel (state 2)."""
    hsx = 42
    t = tile(eng9, tables, "wide-%d-%d" % (W, complex_tile), seed=W + complex_tile, W=W, H=3100, hsx=hsx, hsy=125,
             ci=_wide_ci(W, hsx, complex_tile))
    try:
        t.prepare()
        assert eng9.soil_words_state() == (2 if complex_tile else 1)
        eng9.set_option("grid_blocks_per_cu", 1)
        for pf in (0, 1):
            eng9.set_option("prefetch", pf)
            if what == "one-table":
                for ilp in (1, 2, 4):
                    eng9.set_option("ilp1", ilp)
                    name = run_strip(t, 3, 1 << K1, "ilp1 %d, pipeline %d" % (ilp, pf))
                    assert name == "cn_strip_kernel<1, 3, true, %d, true, %s>" % (ilp, "true" if pf and ilp <= 2 else "false")
            else:
                for ilp in (1, 2):
                    eng9.set_option("ilp16", ilp)
                    tmask = 0x1FF if what == "all-tables" else SUBSET
                    name = run_strip(t, 3, tmask, "ilp16 %d, pipeline %d" % (ilp, pf))
                    assert name == "cn_strip_kernel<0, 3, %s, %d, true, %s>" % (
                        "true" if tmask == 0x1FF else "false", ilp, "true" if pf else "false")
        if what == "one-table":
            # each condition by itself, and the default grid (16 workgroups per CU: one trip, most threads idle)
            eng9.set_option("defaults", 0)
            for cond in (1, 2):
                run_strip(t, cond, 1 << K1, "condition mask %d, default shape" % cond)
    finally:
        t.close()


# ---- few rows ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,hsx", [(1056, 43), (131072, 5243)], ids=["1056", "131072"])
def test_fewer_rows_than_xcds(eng9, tables, W, hsx):
    """Strips of 1, 5 and 9 rows.  131072 columns at one workgroup per CU: the 9-row strip runs on 256 workgroups whose
    XCD shares hold exactly one row each (B = 1: the ninth row is a second trip of one piece), the 5-row strip on 160
    workgroups as one piece, the 1-row strip on 32."""
    t = tile(eng9, tables, "few-%d" % W, seed=W, W=W, H=9, hsx=hsx, hsy=4)
    try:
        t.prepare()
        assert eng9.soil_words_state() == 1
        for per_cu in (1, 16):
            eng9.set_option("grid_blocks_per_cu", per_cu)
            eng9.set_option("ilp1", 1)
            for rows in (1, 5, 9):
                run_strip(t, 1, 1 << K1, "one table, %d rows" % rows, y0=0, rows=rows)
                run_strip(t, 3, 0x1FF, "all tables, %d rows" % rows, y0=9 - rows, rows=rows)
            eng9.set_option("ilp1", 2)
            run_strip(t, 2, 1 << K1, "one table, 9 rows, two sub-trips")
    finally:
        t.close()


# ---- a strip that starts inside a block --------------------------------------------------------------------------

def test_strip_at_row_17_of_a_taller_block(eng9, tables):
    """The strip's landcover, row map and rasters begin at row 17: y0 * W bytes and y0 entries into the block's."""
    t = tile(eng9, tables, "offset", seed=17, W=2064, H=60, hsx=83, hsy=9)
    try:
        t.prepare()
        for rows in (1, 13, 43):
            run_strip(t, 3, 1 << K1, "one table, rows 17..%d" % (17 + rows), y0=17, rows=rows)
            run_strip(t, 3, 0x1FF, "all tables, rows 17..%d" % (17 + rows), y0=17, rows=rows)
            run_strip(t, 1, SUBSET, "three tables, rows 17..%d" % (17 + rows), y0=17, rows=rows)
    finally:
        t.close()


# ---- column maps ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,state", [("A-decreasing", 1), ("A-constant", 1), ("B-runs", 1), ("B-scattered", 2),
                                        ("A-zig-zag", 2), ("C-first", 2), ("C-last", 2), ("D-1x1", 1), ("D-1x4", 1),
                                        ("D-70x1", 1), ("D-narrow-cells", 2)])
def test_column_maps(eng9, tables, name, state):
    """The tiles of the soil-reader cases through the aligned strips: a descending map (c_hi = c_lo - 1 in the groups
    with two cells: the form with two byte loads), columns below 0 and at or above hsx (clamped unsigned), one soil
    column, one soil row, and the tiles with a group that has no compact entry (pixel by pixel)."""
    t = sr.make_tile(eng9, tables, name)
    try:
        t.prepare()
        assert eng9.soil_words_state() == state
        run_strip(t, 3, 1 << K1, name + ", one table")
        run_strip(t, 3, 0x1FF, name + ", all tables")
        run_strip(t, 2, SUBSET, name + ", three tables")
        eng9.set_option("prefetch", 0)
        eng9.set_option("ilp1", 4)
        run_strip(t, 1, 1 << K1, name + ", one table, four sub-trips")
    finally:
        t.close()


def test_descending_map_on_several_trips(eng9, tables):
    """The two-byte-load form over several trips per piece, with row ends in every wave."""
    W, hsx = 1040, 42
    ci = (hsx - 1 - np.arange(W) * hsx // W).astype(np.int32)
    t = tile(eng9, tables, "descending", seed=5, W=W, H=3100, hsx=hsx, hsy=125, ci=ci)
    try:
        t.prepare()
        assert eng9.soil_words_state() == 1
        eng9.set_option("grid_blocks_per_cu", 1)
        eng9.set_option("ilp1", 1)
        run_strip(t, 3, 1 << K1, "one table")
        run_strip(t, 3, 0x1FF, "all tables")
    finally:
        t.close()


# ---- a row with more column groups than the grid has threads ------------------------------------------------------

def test_too_few_threads_for_one_row(eng9, tables):
    """W = 16 * (256 * 256 + 1) on one workgroup per CU: 65536 threads, 65537 column groups.  No lane plan: the strip
    reads the code bytes, made for it, in the same kernels."""
    W = 16 * (256 * 256 + 1)
    t = tile(eng9, tables, "too-wide", seed=9, W=W, H=3, hsx=41944, hsy=2)
    try:
        t.prepare()
        eng9.set_option("grid_blocks_per_cu", 1)
        assert eng9.soil_words_state() == 1
        run_strip(t, 3, 1 << K1, "one table")
        run_strip(t, 3, 0x1FF, "all tables")
        eng9.set_option("grid_blocks_per_cu", 16)       # now every group has its thread
        run_strip(t, 3, 1 << K1, "one table, 16 workgroups per CU")
    finally:
        t.close()


# ---- the snapshot ----------------------------------------------------------------------------------------------------

def test_coarse_and_ci_are_not_read_after_prepare_tile(eng9, tables):
    t = tile(eng9, tables, "snapshot", seed=3, W=2048, H=40, hsx=90, hsy=6)
    try:
        t.prepare()
        eng9.sync()
        eng9.memset(t.bufs[1].ptr, 0xEE, t.coarse.nbytes)
        eng9.memset(t.bufs[2].ptr, 0xEE, t.ci.nbytes)
        eng9.sync()
        assert eng9.soil_words_state() == 1
        run_strip(t, 3, 1 << K1, "one table, caller's buffers overwritten")
        run_strip(t, 3, 0x1FF, "all tables, caller's buffers overwritten")
        run_strip(t, 3, 1 << K1, "rows 17.., caller's buffers overwritten", y0=17)
    finally:
        t.close()
