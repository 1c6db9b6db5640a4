"""What the aggregate tests share: the numpy reduction of a full-resolution raster by the definition of
INTEGRATION.md "Aggregated rasters", and the oracle's rasters of a strip whose soil rows are given by a map.

Never another GPU path: the full-resolution values are the oracle's (oracle/), the reduction is numpy in int64.
"""
import numpy as np

from oracle import cn_oracle_c as oc


def cells(n, f):
    return -(-n // f)


def reduce_sums(raster, x0, x1, f):
    """(s, n, area) of every cell: the sum and the count of the footprint's values != 255, and the footprint's size.
    Cell (cx, cy) covers columns x0 + cx f .. min(x0 + (cx + 1) f, x1) - 1 and rows cy f .. min((cy + 1) f, rows) - 1."""
    v = np.asarray(raster)[:, x0:x1].astype(np.int64)
    ok = v != 255
    ys, xs = np.arange(0, v.shape[0], f), np.arange(0, v.shape[1], f)
    s = np.add.reduceat(np.add.reduceat(np.where(ok, v, 0), ys, axis=0), xs, axis=1)
    n = np.add.reduceat(np.add.reduceat(ok.astype(np.int64), ys, axis=0), xs, axis=1)
    area = np.add.reduceat(np.add.reduceat(np.ones_like(v), ys, axis=0), xs, axis=1)
    return s, n, area


def reduce_raster(raster, x0, x1, f):
    """uint8[ceil(rows / f)][ceil((x1 - x0) / f)]: (2 s + n) // (2 n), 255 where n = 0."""
    s, n, _ = reduce_sums(raster, x0, x1, f)
    out = np.full(s.shape, 255, np.int64)
    np.floor_divide(2 * s + n, 2 * n, out=out, where=n > 0)
    return out.astype(np.uint8)


def oracle_rasters(esa, soil, tables, rasters=range(18)):
    """{r: raster r = condition * 9 + table of the oracle} for landcover esa and the soil class of every pixel."""
    esa = np.ascontiguousarray(esa)
    adj = {}
    out = {}
    for r in rasters:
        c = r // 9
        if c not in adj:
            adj[c] = oc.modify_hysogs_data(np.ascontiguousarray(soil), c == 0)
        out[r] = oc.calculate_cn(esa, adj[c], tables[r % 9]).reshape(esa.shape)
    return out


def selected(cond_mask, table_mask):
    return [c * 9 + k for c in range(2) for k in range(9) if cond_mask >> c & 1 and table_mask >> k & 1]
