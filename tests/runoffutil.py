"""What the tests of the runoff-weighted composites share: the definitions of include/gcn10_host.h "runoff-weighted
composites" in numpy -- the table in np.float64, one operation per line as the header states them, the cell rule in
int64 / Python integers -- and the triples {s, n, sw} of full-resolution rasters over maps, as tests/gridutil.py::add_sums
makes the pairs.  Never another GPU path."""
import numpy as np

from tests import gridutil as gu


def table(P, lam=0.2):
    """uint16[256]: the runoff depth of every raster value in units of 0.01 mm."""
    P, lam = np.float64(P), np.float64(lam)
    v = np.arange(1, 255)
    c = np.minimum(v, 100).astype(np.float64)
    S = np.float64(25400.0) / c - np.float64(254.0)
    Ia = lam * S
    e = P - Ia
    with np.errstate(all="ignore"):
        ee = e * e
        d = e + S
        depth = np.floor(ee / d * np.float64(100.0) + np.float64(0.5))
    q = np.zeros(256, np.int64)
    q[1:255] = np.where(P > Ia, depth, 0.0).astype(np.int64)
    assert q.max() <= 65535
    return q.astype(np.uint16)


def threshold(q):
    """the smallest c with q[c] > 0"""
    return int(np.flatnonzero(np.asarray(q)[:101] > 0)[0])


def cn(s, n, sw, q):
    """The cell rule on Python integers."""
    s, n, sw = int(s), int(n), int(sw)
    if n == 0:
        return 255
    if sw == 0:
        return (2 * s + n) // (2 * n)
    for c in range(1, 100):
        if n * int(q[c]) >= sw:
            return c
    return 100


def cn_array(acc, q):
    """uint8[...] of int64[...][3] triples: the same rule, vectorised (the first c in 1..100 with n q[c] >= sw; triples
    whose products pass 2^63 go through cn())."""
    s, n, sw = acc[..., 0], acc[..., 1], acc[..., 2]
    assert n.max(initial=0) < (1 << 46)
    qq = np.asarray(q, np.int64)[1:101]
    reach = n[..., None] * qq >= sw[..., None]
    reach[..., -1] = True
    out = reach.argmax(axis=-1) + 1
    out = np.where(sw == 0, gu.means(acc[..., :2]).astype(np.int64), out)
    return np.where(n == 0, 255, out).astype(np.uint8)


def add_triples(acc, raster, cellx, celly, w):
    """Adds {sum, count, sum of w[value]} of raster's values != 255 to acc[cy][cx] (int64[ncy][ncx][3]) over the maps
    (-1 = in no cell): gridutil.add_sums with one more word."""
    if np.asarray(raster).size >= gu.BINCOUNT_FROM:
        return gu.add_words_bincount(acc, raster, cellx, celly, w)
    gu.add_sums(acc[:, :, :2], raster, cellx, celly)
    v = np.asarray(raster).astype(np.int64)
    ys, xs = np.flatnonzero(np.asarray(celly) >= 0), np.flatnonzero(np.asarray(cellx) >= 0)
    v = v[np.ix_(ys, xs)]
    cy = np.broadcast_to(np.asarray(celly)[ys][:, None], v.shape)
    cx = np.broadcast_to(np.asarray(cellx)[xs][None, :], v.shape)
    ok = v != 255
    np.add.at(acc[:, :, 2], (cy[ok], cx[ok]), np.asarray(w, np.int64)[v[ok]])
