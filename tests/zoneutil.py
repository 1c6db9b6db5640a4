"""Test helpers of the zonal run mode: the polygon-shapefile writer of gcn10_amd.shapefile and the membership /
ownership rules of include/gcn10_host.h in numpy, evaluated per pixel centre (not per row interval, as the scan
conversion does)."""
import numpy as np

from gcn10_amd.shapefile import write_zone_shapefile  # noqa: F401  (the tests take it from here)


def centres(gt, W, H):
    px = gt[0] + (np.arange(W, dtype=np.float64) + 0.5) * gt[1]
    py = gt[3] + (np.arange(H, dtype=np.float64) + 0.5) * gt[5]
    return px, py


def zone_mask(rings, gt, W, H, with_margin=False):
    """The membership rule per pixel centre: a pixel is in the zone iff the number of crossings c <= px of its row is
    odd (= c[2i] <= px < c[2i+1] for the sorted crossings).  with_margin: also the smallest |px - c| in pixels."""
    px, py = centres(gt, W, H)
    PX, PY = np.meshgrid(px, py)
    count = np.zeros((H, W), np.int64)
    margin = np.inf
    for ring in rings:
        r = [tuple(map(float, p)) for p in ring]
        if r[0] != r[-1]:
            r.append(r[0])
        for (x1, y1), (x2, y2) in zip(r[:-1], r[1:]):
            crosses = (y1 <= PY) != (y2 <= PY)
            if not crosses.any():
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                xc = x1 + (PY - y1) * (x2 - x1) / (y2 - y1)
            count += crosses & (xc <= PX)
            if with_margin:
                margin = min(margin, float(np.abs(PX - xc)[crosses].min()) / abs(gt[1]))
    mask = (count & 1).astype(bool)
    return (mask, margin) if with_margin else mask


def own_mask(gt, W, H, own):
    """The ownership rule: minx <= px < maxx and miny < py <= maxy."""
    px, py = centres(gt, W, H)
    return ((py > own[1]) & (py <= own[3]))[:, None] & ((px >= own[0]) & (px < own[2]))[None, :]


def spans_to_mask(spans, zone, W, H):
    """Mask of one local zone's spans; asserts they are non-empty, inside the window and do not overlap."""
    m = np.zeros((H, W), np.int32)
    for s in spans[spans["zone"] == zone]:
        assert 0 <= s["y"] < H and 0 <= s["x0"] < s["x1"] <= W, s
        m[s["y"], s["x0"]:s["x1"]] += 1
    assert m.max() <= 1
    return m.astype(bool)
