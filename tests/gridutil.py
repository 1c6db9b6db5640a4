"""What the tests of the model-grid run mode share: the membership rule of include/gcn10_host.h "model grid" in numpy
on np.float64 -- the same expressions, the same comparisons --, the plan of a block by that rule, and the sums and
means of full-resolution rasters over maps with np.add.at in int64 (np.bincount from two million pixels on).  Never
another GPU path."""
import numpy as np

from tests import zoneutil


def edges(grid):
    """ex(k) = xmin + k * dx for k = 0 .. nx and ey(k) = ymax - k * dy for k = 0 .. ny: a product, then a sum."""
    ex = np.float64(grid["xmin"]) + np.arange(grid["nx"] + 1, dtype=np.float64) * np.float64(grid["dx"])
    ey = np.float64(grid["ymax"]) - np.arange(grid["ny"] + 1, dtype=np.float64) * np.float64(grid["dy"])
    return ex, ey


def cells_dense(grid, gt, W, H):
    """(column of every pixel column, row of every pixel row) in the grid, -1 = in none: every centre against every
    cell, by the rule as it is written.  For small windows."""
    ex, ey = edges(grid)
    px, py = zoneutil.centres(gt, W, H)
    in_col = (ex[:-1, None] <= px[None, :]) & (px[None, :] < ex[1:, None])          # [nx][W]
    in_row = (ey[1:, None] < py[None, :]) & (py[None, :] <= ey[:-1, None])          # [ny][H]
    assert (in_col.sum(axis=0) <= 1).all() and (in_row.sum(axis=0) <= 1).all()      # a centre is in one cell at most
    kx = np.where(in_col.any(axis=0), in_col.argmax(axis=0), -1)
    ky = np.where(in_row.any(axis=0), in_row.argmax(axis=0), -1)
    return kx.astype(np.int64), ky.astype(np.int64)


def cells(grid, gt, W, H):
    """The same by bisection over the edges (they never decrease): the largest k with ex(k) <= px, the largest k with
    ey(k) >= py, and -1 outside [0, nx) and [0, ny)."""
    ex, ey = edges(grid)
    px, py = zoneutil.centres(gt, W, H)
    kx = np.searchsorted(ex, px, side="right") - 1
    ky = np.searchsorted(-ey, -py, side="right") - 1
    kx = np.where((kx >= 0) & (kx < grid["nx"]), kx, -1)
    ky = np.where((ky >= 0) & (ky < grid["ny"]), ky, -1)
    return kx.astype(np.int64), ky.astype(np.int64)


def plan(grid, gt, W, H, own=None, dense=False):
    """The plan of a block by the rule: the dict of host.grid_plan_block."""
    kx, ky = (cells_dense if dense else cells)(grid, gt, W, H)
    px, py = zoneutil.centres(gt, W, H)
    if own is not None:
        kx = np.where((px >= own[0]) & (px < own[2]), kx, -1)
        ky = np.where((py > own[1]) & (py <= own[3]), ky, -1)
        ox, oy = np.flatnonzero((px >= own[0]) & (px < own[2])), np.flatnonzero((py > own[1]) & (py <= own[3]))
        out = dict(x0=int(ox[0]) if ox.size else 0, x1=int(ox[-1]) + 1 if ox.size else 0,
                   y0=int(oy[0]) if oy.size else 0, y1=int(oy[-1]) + 1 if oy.size else 0)
    else:
        out = dict(x0=0, x1=W, y0=0, y1=H)
    if not (kx >= 0).any() or not (ky >= 0).any():
        out.update(cx0=0, cx1=0, cy0=0, cy1=0, cellx=np.zeros(0, np.int32), celly=np.zeros(0, np.int32),
                   complete_x=np.zeros(0, bool), complete_y=np.zeros(0, bool), shared=np.zeros(0, np.uint32))
        return out
    cx0, cx1 = int(kx[kx >= 0].min()), int(kx.max()) + 1
    cy0, cy1 = int(ky[ky >= 0].min()), int(ky.max()) + 1
    ex, ey = edges(grid)
    if own is not None:
        comp_x = (own[0] <= ex[cx0:cx1]) & (ex[cx0 + 1:cx1 + 1] <= own[2])
        comp_y = (own[1] <= ey[cy0 + 1:cy1 + 1]) & (ey[cy0:cy1] <= own[3])
    else:
        comp_x, comp_y = np.zeros(cx1 - cx0, bool), np.zeros(cy1 - cy0, bool)
    complete = comp_y[:, None] & comp_x[None, :]
    out.update(cx0=cx0, cx1=cx1, cy0=cy0, cy1=cy1, cellx=np.where(kx >= 0, kx - cx0, -1).astype(np.int32),
               celly=np.where(ky >= 0, ky - cy0, -1).astype(np.int32), complete_x=comp_x, complete_y=comp_y,
               shared=np.flatnonzero(~complete.reshape(-1)).astype(np.uint32))
    return out


def same_plan(got, want):
    for k in ("x0", "x1", "y0", "y1", "cx0", "cx1", "cy0", "cy1"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("cellx", "celly", "complete_x", "complete_y", "shared"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


BINCOUNT_FROM = 2000000      # pixels from which add_sums and runoffutil.add_triples count with np.bincount


def add_words_bincount(acc, raster, cellx, celly, w=None):
    """The fast path of add_sums (and, with the weights w, of runoffutil.add_triples) for rasters of millions of pixels,
    where np.add.at takes seconds per word: np.bincount over celly[:, None] * ncx + cellx[None, :] of the pixels that
    are in a cell and != 255.  Weighted bincounts add in float64; every term is an integer and every sum is asserted
    to stay below 2^53, so they are exact and the int64 words are those of np.add.at."""
    ncy, ncx = acc.shape[:2]
    cx, cy = np.asarray(cellx, np.int64), np.asarray(celly, np.int64)
    ys, xs = np.flatnonzero(cy >= 0), np.flatnonzero(cx >= 0)
    v = np.asarray(raster)[np.ix_(ys, xs)]
    cell = (cy[ys][:, None] * ncx + cx[xs][None, :]).astype(np.int32 if ncy * ncx < (1 << 31) else np.int64)
    ok = v != 255
    cell, v = cell[ok], v[ok]
    words = [v.astype(np.float64), None] + ([np.asarray(w, np.float64)[v]] if w is not None else [])
    for k, weights in enumerate(words):
        assert weights is None or float(weights.sum()) < float(1 << 53)
        acc[:, :, k] += np.bincount(cell, weights=weights, minlength=ncy * ncx).astype(np.int64).reshape(ncy, ncx)


def add_sums(acc, raster, cellx, celly):
    """Adds the sum and the count of raster's values != 255 to acc[cy][cx] = {s, n} (int64[ncy][ncx][2]) over the maps
    (-1 = in no cell)."""
    if np.asarray(raster).size >= BINCOUNT_FROM:
        return add_words_bincount(acc, raster, cellx, celly)
    v = np.asarray(raster).astype(np.int64)
    ys, xs = np.flatnonzero(np.asarray(celly) >= 0), np.flatnonzero(np.asarray(cellx) >= 0)
    v = v[np.ix_(ys, xs)]
    cy = np.broadcast_to(np.asarray(celly)[ys][:, None], v.shape)
    cx = np.broadcast_to(np.asarray(cellx)[xs][None, :], v.shape)
    ok = v != 255
    np.add.at(acc[:, :, 0], (cy[ok], cx[ok]), v[ok])
    np.add.at(acc[:, :, 1], (cy[ok], cx[ok]), 1)


def means(acc):
    """uint8: (2 s + n) // (2 n), 255 where n = 0, of int64[...][2] pairs."""
    s, n = acc[..., 0], acc[..., 1]
    out = np.full(s.shape, 255, np.int64)
    np.floor_divide(2 * s + n, 2 * n, out=out, where=n > 0)
    return out.astype(np.uint8)
