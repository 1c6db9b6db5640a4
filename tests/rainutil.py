"""What the tests of the rainfall raster share: the definition of include/gcn10_gpu.h "a weight table per cell" in numpy.
For every pixel the raster value comes from the oracle; the triples {s, n, sw} are added per (celly, cellx) with
np.bincount in int64 -- sw from the table the cell's byte names, an entry >= k counting as table 0 --, and the bytes come
from runoffutil.cn, cell by cell, with the cell's own table.  Never another GPU path."""
import numpy as np

from tests import gridutil as gu
from tests import runoffutil as ru


def tables_256(unit=2.5, lam=0.2, seed=11):
    """uint16[256][256], all different: table b is the runoff table of b * unit mm, but every fourth one (b % 4 == 3)
    is random, so that it decreases somewhere and takes the scan of the finish pass."""
    rng = np.random.default_rng(seed)
    t = np.stack([ru.table(b * unit, lam) if b % 4 != 3 else rng.integers(0, 65536, 256).astype(np.uint16)
                  for b in range(256)])
    assert len({row.tobytes() for row in t}) == 256
    return t


def clamp_field(field, k):
    """the table every cell counts with: its byte, 0 where the byte names no table"""
    f = np.asarray(field, np.int64)
    return np.where(f < k, f, 0)


def valid_maps(cellx, celly, ncx, ncy):
    """the maps with every entry outside [0, ncx) and [0, ncy) as -1, in int64"""
    cx, cy = np.asarray(cellx, np.int64), np.asarray(celly, np.int64)
    return np.where((cx >= 0) & (cx < ncx), cx, -1), np.where((cy >= 0) & (cy < ncy), cy, -1)


def add_triples(acc, raster, cellx, celly, field, tables):
    """Adds {sum, count, sum of tables[field[cy][cx]][value]} of raster's values != 255 to acc[cy][cx]
    (int64[ncy][ncx][3]) over the maps (anything outside the cells = in no cell).  Weighted bincounts add in float64;
    every term is an integer and every sum is asserted to stay below 2^53, so they are exact."""
    ncy, ncx = acc.shape[:2]
    cx, cy = valid_maps(cellx, celly, ncx, ncy)
    ys, xs = np.flatnonzero(cy >= 0), np.flatnonzero(cx >= 0)
    v = np.asarray(raster)[np.ix_(ys, xs)]
    cell = cy[ys][:, None] * ncx + cx[xs][None, :]
    ok = v != 255
    cell, v = cell[ok], v[ok].astype(np.int64)
    of_cell = clamp_field(field, len(tables)).reshape(-1)
    w = np.asarray(tables, np.float64)[of_cell[cell], v]
    for k, weights in enumerate((v.astype(np.float64), None, w)):
        assert weights is None or float(weights.sum()) < float(1 << 53)
        acc[:, :, k] += np.bincount(cell, weights=weights, minlength=ncy * ncx).astype(np.int64).reshape(ncy, ncx)


def cn_cells(acc, field, tables):
    """uint8[...]: runoffutil.cn of every triple of int64[n_sel][n_cells][3] with the table of its cell (field[n_cells])"""
    of_cell = clamp_field(field, len(tables)).reshape(-1)
    out = np.empty(acc.shape[:2], np.uint8)
    for q in range(acc.shape[0]):
        for c in range(acc.shape[1]):
            out[q, c] = ru.cn(acc[q, c, 0], acc[q, c, 1], acc[q, c, 2], tables[of_cell[c]])
    return out


def means(acc):
    return gu.means(acc[..., :2])
