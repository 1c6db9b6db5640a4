"""GPU: what the entry points that read the soil of a prepared tile answer BEFORE they launch anything -- the state
and argument checks they share (gcn10::check_tables / bind_soil / check_masks of gcn10_gpu_internal.hpp) -- and that
a refused call leaves the context fit for the next good one.  Needs an MI355X.

The entry points: gcn10_gpu_cn_strip (at this width it launches the byte strip kernel; the vector kernel is behind
the same preamble), gcn10_gpu_verify_strip, gcn10_gpu_pair_histogram, gcn10_gpu_zonal_pair_histogram,
gcn10_gpu_overview_average, gcn10_gpu_deflate_fused_strip, gcn10_gpu_aggregate and gcn10_gpu_grid_sums (its weighted
and storms forms are behind the same preamble, after a check of the weights).  For each of them, on a context of its
own, so that the call is the first one after the state it tests:

  (a) tables loaded, no tile prepared                      GCN10_E_STATE
  (b) tile prepared for W = 32, called with W = 48         GCN10_E_INVAL from gcn10_gpu_cn_strip (a bad argument
                                                           there), GCN10_E_STATE from the others
  (c) cond_mask 0 and 4, table_mask 0 and 1 << 9           GCN10_E_INVAL (the six entries that take masks)
  (d) rows == 0 with null pointers                         success from cn_strip, verify_strip and deflate_fused_strip;
                                                           GCN10_E_INVAL from pair_histogram (it looks at its
                                                           pointers first; success with pointers) and from
                                                           overview_average, aggregate and grid_sums (an empty
                                                           strip is a bad strip there);
                                                           zonal: n_items == 0 is success whatever else it is given,
                                                           even without a tile
  (e) after each of these, the same context runs the reader of tests/soil_readers.py for that entry point, whose
      result is compared with the oracle / numpy references there.

The codes of the first six are those of the code before the preamble was shared
(profiles/soil_view/preamble_on_parent.txt: this module run against that library); gcn10_gpu_aggregate came after
it, and its codes are the ones tests/test_gpu_aggregate.py::test_errors pins, as gcn10_gpu_grid_sums has those of
tests/test_gpu_grid.py::test_errors.  Shapes: the smallest that reach every
check -- a tile of 32 x 2 pixels over a 2 x 2 soil window, one strip of 2 rows.
"""
import ctypes as C

import numpy as np
import pytest

from gcn10_amd import gpu
from tests import soil_readers as sr

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_STATE = 0, -1, -4
W, H, HS = 32, 2, 2
OTHER_W = 48
SLOT = 256
WITH_MASKS = ("strip", "verify", "overview", "fused", "aggregate", "grid")
NAMES = {"strip": "gcn10_gpu_cn_strip", "verify": "gcn10_gpu_verify_strip", "histogram": "gcn10_gpu_pair_histogram",
         "zonal": "gcn10_gpu_zonal_pair_histogram", "overview": "gcn10_gpu_overview_average",
         "fused": "gcn10_gpu_deflate_fused_strip", "aggregate": "gcn10_gpu_aggregate", "grid": "gcn10_gpu_grid_sums"}


@pytest.fixture
def ctx(tables):
    """A context of its own with the tables loaded and no tile prepared, and the tile's inputs on the device."""
    eng = gpu.Engine(0)
    try:
        eng.set_tables(tables)
        tile = sr.ReaderTile(eng, tables, seed=77, W=W, H=H, hsx=HS, hsy=HS, key="preamble-32x2")
        scratch = eng.alloc(20 * SLOT)      # whatever a refused or empty call is handed besides the tile's inputs
        eng.memset(scratch.ptr, 0, 20 * SLOT)
        eng.sync()
        yield eng, tile, scratch
        eng.sync()
    finally:
        eng.close()


def call(reader, eng, tile, scratch, w=W, rows=H, cond=3, table=0x1FF, null=False, n_items=1):
    """The return code of one call of the entry point; with null = True every pointer argument is null."""
    L, c = gpu.lib(), eng._ctx
    esa, cj = (None, None) if null else (tile.bufs[0].ptr, tile.bufs[3].ptr)
    at = (lambda i: None) if null else (lambda i: scratch.ptr + i * SLOT)
    ptrs = None if null else (C.c_void_p * 18)(*[at(r) for r in range(18)])
    if reader == "strip":
        return L.gcn10_gpu_cn_strip(c, esa, w, rows, cj, cond, table, ptrs, None)
    if reader == "verify":
        return L.gcn10_gpu_verify_strip(c, esa, w, rows, cj, cond, table, ptrs, max(w, 1), 0, at(18), None)
    if reader == "histogram":
        return L.gcn10_gpu_pair_histogram(c, esa, w, rows, cj, at(0), None)
    if reader == "zonal":
        return L.gcn10_gpu_zonal_pair_histogram(c, esa, w, rows, cj, at(0), at(1), n_items, 1, at(2), None)
    if reader == "overview":
        return L.gcn10_gpu_overview_average(c, esa, w, rows, 0, rows, cj, cond, table, 1, ptrs, None)
    if reader == "fused":
        return L.gcn10_gpu_deflate_fused_strip(c, esa, w, rows, cj, cond, table, at(0), 16 * SLOT, at(17), at(18), None)
    if reader == "aggregate":           # cells of 2 x 2 px over all columns: one row of w / 2 cells in a slot
        return L.gcn10_gpu_aggregate(c, esa, w, rows, cj, 0, w, 2, cond, table, ptrs, SLOT, None)
    assert reader == "grid"             # one cell (the maps are the scratch's zeros), its 18 pairs in slots 2 and 3
    return L.gcn10_gpu_grid_sums(c, esa, w, rows, cj, at(0), at(1), 1, 1, cond, table, at(2), None)


def refused(code, reader, rc, about=None):
    msg = gpu.lib().gcn10_gpu_last_error().decode()
    assert rc == code, "%s returned %d (%s)" % (NAMES[reader], rc, msg)
    assert NAMES[reader] in msg, msg
    if about:
        assert about in msg, msg


def good_call(eng, tile, reader):
    """(e): the context still works -- the reader's own launch and check against the references."""
    eng.sync()
    sr.run_reader(tile, reader)


@pytest.mark.parametrize("reader", sr.READERS)
def test_a_no_tile_prepared(ctx, reader):
    eng, tile, scratch = ctx
    try:
        refused(E_STATE, reader, call(reader, eng, tile, scratch), about="prepare")
        tile.prepare()
        good_call(eng, tile, reader)
    finally:
        eng.sync()
        tile.close()


@pytest.mark.parametrize("reader", sr.READERS)
def test_b_another_width_than_the_prepared_tiles(ctx, reader):
    eng, tile, scratch = ctx
    try:
        tile.prepare()
        code = E_INVAL if reader == "strip" else E_STATE
        refused(code, reader, call(reader, eng, tile, scratch, w=OTHER_W), about="prepare")
        good_call(eng, tile, reader)
    finally:
        eng.sync()
        tile.close()


@pytest.mark.parametrize("reader", WITH_MASKS)
def test_c_masks_out_of_range(ctx, reader):
    eng, tile, scratch = ctx
    try:
        tile.prepare()
        for cond, table in ((0, 0x1FF), (4, 0x1FF), (3, 0), (3, 1 << 9)):
            refused(E_INVAL, reader, call(reader, eng, tile, scratch, cond=cond, table=table))
        good_call(eng, tile, reader)
    finally:
        eng.sync()
        tile.close()


@pytest.mark.parametrize("reader", sr.READERS)
def test_d_an_empty_strip(ctx, reader):
    eng, tile, scratch = ctx
    try:
        if reader == "zonal":
            # no items: nothing to do, before any other check -- no tile, no pointers
            assert call(reader, eng, tile, scratch, null=True, n_items=0) == OK
            assert call(reader, eng, tile, scratch, w=OTHER_W, null=True, n_items=0) == OK
            tile.prepare()
            assert call(reader, eng, tile, scratch, null=True, n_items=0) == OK
        else:
            tile.prepare()
            rc = call(reader, eng, tile, scratch, rows=0, null=True)
            if reader in ("histogram", "overview", "aggregate", "grid"):
                refused(E_INVAL, reader, rc)
            else:
                assert rc == OK, gpu.lib().gcn10_gpu_last_error().decode()
            if reader == "histogram":
                assert call(reader, eng, tile, scratch, rows=0) == OK
                eng.sync()
                assert not eng.download(scratch.ptr, (SLOT,)).any(), "an empty strip was counted"
        good_call(eng, tile, reader)     # (syncs first: whatever the empty call launched has run without a fault)
    finally:
        eng.sync()
        tile.close()
