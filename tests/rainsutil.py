"""What the tests of several rainfall rasters in one run share (config key rains, gcn10_gpu_grid_sums_rains,
gcn10_gpu_grid_finish_rains): the words {s, n, sw_1 .. sw_k} of include/gcn10_gpu.h "several weight tables per cell" put
together from the restatements the one-raster tests use -- words 0 and 1 from tests/gridutil.py, word 2 + j from
rainutil.add_triples with field j, the bytes from rainutil.cn_cells with field j --, and the runs of the two calls with
poison around everything they write.  Never another GPU path."""
import numpy as np

from tests import aggutil as au
from tests import gridutil as gu
from tests import rainutil as rn

POISON, GUARD = 0xA5, 256


def fields_for(k, ncx, ncy, seed=3):
    """uint8[k][ncy][ncx], random and different from layer to layer, with all 256 values in every layer of 256 cells or
    more (the recipe of tests/test_gpu_grid_rain.py::field_for, layer j from seed + 2 j)"""
    out = []
    for j in range(k):
        f = np.random.default_rng(seed + 2 * j).integers(0, 256, (ncy, ncx)).astype(np.uint8)
        if f.size >= 256:
            at = np.random.default_rng(seed + 2 * j + 1).permutation(f.size)[:256]
            f.reshape(-1)[at] = np.arange(256, dtype=np.uint8)
        out.append(f)
    out = np.stack(out)
    assert k == 1 or ncx * ncy < 4 or all((out[0] != out[j]).any() for j in range(1, k))
    return out


def want_words(inp, cellx, celly, fields, tables, cond_mask=3, table_mask=0x1FF):
    """int64[n_sel][ncy][ncx][2 + k] of the oracle's rasters over the maps (anything outside the cells = in no cell)"""
    fields = np.asarray(fields)
    k, ncy, ncx = fields.shape
    sel = au.selected(cond_mask, table_mask)
    cx, cy = rn.valid_maps(cellx, celly, ncx, ncy)
    acc = np.zeros((len(sel), ncy, ncx, 2 + k), np.int64)
    for q, r in enumerate(sel):
        raster = inp.want(r)[:len(celly)]
        pair = np.zeros((ncy, ncx, 2), np.int64)
        gu.add_words_bincount(pair, raster, cx, cy)
        acc[q, :, :, :2] = pair
        for j in range(k):
            triple = np.zeros((ncy, ncx, 3), np.int64)
            rn.add_triples(triple, raster, cellx, celly, fields[j], tables)
            assert (triple[:, :, :2] == pair).all()             # the two restatements agree on what they share
            acc[q, :, :, 2 + j] = triple[:, :, 2]
    return acc


def run_rains(sc, cellx, celly, fields, tables, cond_mask=3, table_mask=0x1FF, bands=None, repeat=1):
    """int64[n_sel][ncy][ncx][2 + k] after set_rain_tables(tables) and grid_sums_rains over the scene's strip with the
    fields uint8[k][ncy][ncx], uploaded into exactly k * ncy * ncx bytes -- in one call, or one call per (y0, rows) of
    `bands` --, `repeat` times; asserts that not a byte around the words was written."""
    inp, eng = sc.inp, sc.eng
    fields = np.ascontiguousarray(fields, np.uint8)
    k, ncy, ncx = fields.shape
    sel = au.selected(cond_mask, table_mask)
    nbytes = len(sel) * ncy * ncx * 8 * (2 + k)
    buf = eng.alloc(nbytes + 2 * GUARD)
    ups = [eng.upload(np.ascontiguousarray(cellx, np.int32)), eng.upload(np.ascontiguousarray(celly, np.int32)),
           eng.upload(fields)]
    assert ups[2].nbytes == k * ncy * ncx
    try:
        eng.set_rain_tables(tables)
        eng.memset(buf.ptr, POISON, nbytes + 2 * GUARD)
        eng.memset(buf.ptr + GUARD, 0, nbytes)
        for _rep in range(repeat):
            for y0, n in bands or [(0, len(celly))]:
                eng.grid_sums_rains(sc.esa_ptr + y0 * inp.W, inp.W, n, sc.bufs[3].ptr + 4 * y0, ups[0].ptr,
                                    ups[1].ptr + 4 * y0, ncx, ncy, cond_mask, table_mask, ups[2].ptr, k,
                                    buf.ptr + GUARD)
        eng.sync()
        img = eng.download(buf.ptr, (nbytes + 2 * GUARD,))
    finally:
        eng.sync()
        for b in [buf] + ups:
            b.close()
    assert (img[:GUARD] == POISON).all() and (img[GUARD + nbytes:] == POISON).all(), "bytes around acc were written"
    return img[GUARD:GUARD + nbytes].view(np.uint64).astype(np.int64).reshape(len(sel), ncy, ncx, 2 + k)


def same_words(got, want, what=""):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d of %d words differ, first (q, cy, cx, word) = %s: got %d, want %d" % (
        what, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def check_rains(sc, cellx, celly, fields, tables, cond_mask=3, table_mask=0x1FF, **kw):
    got = run_rains(sc, cellx, celly, fields, tables, cond_mask, table_mask, **kw)
    same_words(got, want_words(sc.inp, cellx, celly, fields, tables, cond_mask, table_mask), "W=%d" % sc.inp.W)
    return got


def run_finish_rains(eng, acc, fields, tables, shared_idx):
    """(means uint8[n_sel][n_cells], cnq uint8[k][n_sel][n_cells], shared int64[n_sel][n_shared][2 + k]) of
    set_rain_tables(tables) and grid_finish_rains over int64 words [n_sel][n_cells][2 + k] with fields uint8[k][n_cells];
    asserts that not a byte around the three was written."""
    n_sel, n_cells, words = acc.shape
    k = words - 2
    fields = np.ascontiguousarray(fields, np.uint8).reshape(k, n_cells)
    idx = np.asarray(shared_idx, np.uint32)
    n_sh, nb = len(idx), n_sel * n_cells
    d_acc = eng.upload(np.ascontiguousarray(acc).astype(np.uint64))
    d_fields = eng.upload(fields)
    d_idx = eng.upload(idx) if n_sh else None
    out = [eng.alloc(nb + 2 * GUARD), eng.alloc(k * nb + 2 * GUARD), eng.alloc(n_sel * n_sh * 8 * words + 2 * GUARD)]
    try:
        eng.set_rain_tables(tables)
        for b in out:
            eng.memset(b.ptr, POISON, b.nbytes)
        eng.grid_finish_rains(d_acc.ptr, n_sel, n_cells, d_fields.ptr, k, out[0].ptr + GUARD, out[1].ptr + GUARD,
                              d_idx.ptr if n_sh else None, n_sh, out[2].ptr + GUARD if n_sh else None)
        eng.sync()
        img = [eng.download(b.ptr, (b.nbytes,)) for b in out]
    finally:
        eng.sync()
        for b in [d_acc, d_fields, d_idx] + out:
            if b is not None:
                b.close()
    for name, im in zip(("means", "cnq", "shared"), img):
        assert (im[:GUARD] == POISON).all() and (im[-GUARD:] == POISON).all(), "bytes around %s were written" % name
    return (img[0][GUARD:-GUARD].reshape(n_sel, n_cells), img[1][GUARD:-GUARD].reshape(k, n_sel, n_cells),
            img[2][GUARD:-GUARD].view(np.uint64).astype(np.int64).reshape(n_sel, n_sh, words))


def want_bytes(acc, fields, tables):
    """(means, cnq uint8[k][n_sel][n_cells]) of int64 words [n_sel][n_cells][2 + k]: gridutil.means of words 0 and 1,
    and rainutil.cn_cells of {word 0, word 1, word 2 + j} with field j"""
    k = acc.shape[2] - 2
    fields = np.asarray(fields).reshape(k, -1)
    cnq = np.stack([rn.cn_cells(acc[:, :, [0, 1, 2 + j]], fields[j], tables) for j in range(k)])
    return gu.means(acc[..., :2]), cnq
