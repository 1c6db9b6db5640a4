"""What the tests of several design storms share: sets of weight tables built from the adversarial tables of
tests/test_gpu_grid_runoff.py and the real tables of 25 / 50 / 100 mm, and the 2 + k words {s, n, sw_0, ..., sw_(k-1)} of
full-resolution rasters over maps, in numpy int64.  add_words counts every table over one set of cell indices with
np.bincount (exact: every term is an integer and every sum is asserted to stay below 2^53, as in
gridutil.add_words_bincount); tests/test_storms_host.py holds it to runoffutil.add_triples.  Never another GPU path."""
import numpy as np

from tests import runoffutil as ru

KS = (1, 2, 3, 8)
ADVERSARIAL = ("low bytes 255", "high bytes 255", "all 65535", "random")
POOL = {
    "low bytes 255": np.full(256, 0x00FF, np.uint16),
    "high bytes 255": np.full(256, 0xFF00, np.uint16),
    "all 65535": np.full(256, 0xFFFF, np.uint16),
    "random": np.random.default_rng(5).integers(0, 65536, 256).astype(np.uint16),
    "25 mm": ru.table(25, 0.2),
    "50 mm": ru.table(50, 0.2),
    "100 mm": ru.table(100, 0.2),
}
ORDER = ("low bytes 255", "25 mm", "high bytes 255", "50 mm", "all 65535", "100 mm", "random")


def table_names(k, turn):
    """the names of a set of k tables: ORDER from `turn` on, round and round"""
    return [ORDER[(turn + j) % len(ORDER)] for j in range(k)]


def table_set(k, turn):
    """uint16[k][256]"""
    return np.stack([POOL[name] for name in table_names(k, turn)])


def add_words(acc, raster, cellx, celly, ws):
    """Adds {sum, count, sum of ws[0][value], sum of ws[1][value], ...} of raster's values != 255 to acc[cy][cx]
    (int64[ncy][ncx][2 + k]) over the maps (-1 = in no cell)."""
    ncy, ncx = acc.shape[:2]
    cx, cy = np.asarray(cellx, np.int64), np.asarray(celly, np.int64)
    ys, xs = np.flatnonzero(cy >= 0), np.flatnonzero(cx >= 0)
    v = np.asarray(raster)[np.ix_(ys, xs)]
    cell = (cy[ys][:, None] * ncx + cx[xs][None, :])
    ok = v != 255
    cell, v = cell[ok], v[ok]
    words = [v.astype(np.float64), None] + [np.asarray(w, np.float64)[v] for w in ws]
    assert acc.shape[2] == len(words)
    for k, weights in enumerate(words):
        assert weights is None or float(weights.sum()) < float(1 << 53)
        acc[:, :, k] += np.bincount(cell, weights=weights, minlength=ncy * ncx).astype(np.int64).reshape(ncy, ncx)


def cn_arrays(acc, ws):
    """uint8[k][...] of int64[...][2 + k] words: runoffutil.cn_array per table"""
    return np.stack([ru.cn_array(acc[..., [0, 1, 2 + j]], w) for j, w in enumerate(ws)])
