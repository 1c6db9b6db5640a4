"""Test helpers of the zonal run mode: the polygon-shapefile writer of gcn10_amd.shapefile and the membership /
ownership rules of include/gcn10_host.h in numpy, evaluated per pixel centre (not per row interval, as the scan
conversion does); vertices on pixel centres, a triangulated lattice of them, coverage of a plan's spans, and the
membership in exact rational arithmetic."""
import math
import struct
from fractions import Fraction

import numpy as np

from gcn10_amd.shapefile import write_zone_shapefile  # noqa: F401  (the tests take it from here)

PX = 8.3333333333330430e-05                 # the landcover's pixel
# a plain one, an origin off the pixel grid by rounding, and the real pixel where ulp(px) is largest
TIE_GTS = [[12.3, 0.0125, 0.0, 48.7, 0.0, -0.0075],
           [-111.0000000000024, PX, 0.0, 39.00000000000157, 0.0, -PX],
           [179.9, PX, 0.0, -59.9, 0.0, -PX]]


def centres(gt, W, H):
    px = gt[0] + (np.arange(W, dtype=np.float64) + 0.5) * gt[1]
    py = gt[3] + (np.arange(H, dtype=np.float64) + 0.5) * gt[5]
    return px, py


def zone_mask(rings, gt, W, H, with_margin=False):
    """The membership rule per pixel centre: a pixel is in the zone iff the number of crossings c <= px of its row is
    odd (= c[2i] <= px < c[2i+1] for the sorted crossings), every crossing evaluated from the edge's lower endpoint.
    with_margin: also the smallest |px - c| in pixels."""
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
            (xl, yl), (xh, yh) = ((x1, y1), (x2, y2)) if y1 < y2 else ((x2, y2), (x1, y1))
            with np.errstate(divide="ignore", invalid="ignore"):
                xc = xl + (PY - yl) * (xh - xl) / (yh - yl)
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


def coverage(spans, W, H):
    """How many spans name each pixel, int32[H][W]; asserts they are non-empty and inside the window."""
    assert ((0 <= spans["y"]) & (spans["y"] < H) & (0 <= spans["x0"]) & (spans["x0"] < spans["x1"]) &
            (spans["x1"] <= W)).all()
    d = np.zeros((H, W + 1), np.int32)
    np.add.at(d, (spans["y"], spans["x0"]), 1)
    np.add.at(d, (spans["y"], spans["x1"]), -1)
    return np.cumsum(d, axis=1)[:, :W]


def spans_by_record(plan, n_records):
    """The plan's spans per record of the file (a record without pixels: an empty array)."""
    spans = plan["spans"]
    cuts = np.searchsorted(spans["zone"], np.arange(len(plan["local_zone"]) + 1))
    out = [spans[:0]] * n_records
    for li, zi in enumerate(plan["local_zone"].tolist()):
        out[zi] = spans[cuts[li]:cuts[li + 1]]
    return out


def pt(gt, u, v):
    """The point u, v pixels from the centre of pixel (0, 0): for integers, the centre of pixel (u, v) as the rule
    computes it."""
    return (gt[0] + (u + 0.5) * gt[1], gt[3] + (v + 0.5) * gt[5])


def on_centres(gt, uv):
    return [pt(gt, u, v) for u, v in uv]


def lattice_triangles(gt, u0, v0, nx, ny, sx, sy, seed):
    """A lattice of (nx + 1) x (ny + 1) vertices on the centres of pixels (u0 + i sx, v0 + j sy), each cell split into
    two triangles along a diagonal chosen by a seeded coin, each triangle written clockwise or counter-clockwise from
    a seeded vertex.  Returns the triangles' rings (one zone each) and the pixels the rule gives to the hull,
    (x0, x1, y0, y1): columns [x0, x1) and rows [y0, y1)."""
    rng = np.random.default_rng(seed)
    rings = []
    for j in range(ny):
        for i in range(nx):
            a, b = (u0 + i * sx, v0 + j * sy), (u0 + (i + 1) * sx, v0 + j * sy)
            c, d = (u0 + (i + 1) * sx, v0 + (j + 1) * sy), (u0 + i * sx, v0 + (j + 1) * sy)
            for tri in ([a, b, c], [a, c, d]) if rng.integers(0, 2) else ([a, b, d], [b, c, d]):
                k = int(rng.integers(0, 3))
                tri = tri[k:] + tri[:k]
                rings.append(on_centres(gt, tri[::-1] if rng.integers(0, 2) else tri))
    # ymin <= py < ymax: the top row of vertices is out, the bottom one in; xmin <= px < xmax
    return rings, (u0, u0 + nx * sx, v0 + 1, v0 + ny * sy + 1)


def hull_mask(gt, W, H, rings):
    """The pixels the rule gives to the bounding rectangle of the rings' points, by comparisons of the centres."""
    xs = [p[0] for r in rings for p in r]
    ys = [p[1] for r in rings for p in r]
    px, py = centres(gt, W, H)
    return ((min(ys) <= py) & (py < max(ys)))[:, None] & ((min(xs) <= px) & (px < max(xs)))[None, :]


def polygon_record(rings, shape_type=5):
    """The content of a polygon record with the rings exactly as given (write_zone_shapefile closes them)."""
    pts = [p for r in rings for p in r]
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    c = struct.pack("<i4d2i", shape_type, min(xs), min(ys), max(xs), max(ys), len(rings), len(pts))
    at = 0
    for r in rings:
        c += struct.pack("<i", at)
        at += len(r)
    return c + b"".join(struct.pack("<2d", float(x), float(y)) for x, y in pts)


def ulp_of(m):
    """ulp of the double nearest to the magnitude m (a Fraction or a float)"""
    return Fraction(math.ulp(float(m)))


def exact_membership(rings, gt, W, H, ulps):
    """Even-odd membership of every pixel centre in exact rational arithmetic on the very doubles, and the pixels
    nearer to a crossing c of their row than E = ulps * ulp(max(|c|, |c - xl|)), xl the x of the edge's lower
    endpoint.  Returns (inside, near), bool[H][W] each."""
    px, py = centres(gt, W, H)
    pxf = [Fraction(float(v)) for v in px]
    toggle = np.zeros((H, W + 1), np.int64)
    near = np.zeros((H, W), bool)
    for ring in rings:
        r = [tuple(map(float, p)) for p in ring]
        if r[0] != r[-1]:
            r.append(r[0])
        for (x1, y1), (x2, y2) in zip(r[:-1], r[1:]):
            if y1 == y2:
                continue
            (xl, yl), (xh, yh) = ((x1, y1), (x2, y2)) if y1 < y2 else ((x2, y2), (x1, y1))
            fxl, fyl, fxh, fyh = Fraction(xl), Fraction(yl), Fraction(xh), Fraction(yh)
            for y in np.nonzero((yl <= py) & (py < yh))[0].tolist():        # comparisons of doubles are exact
                c = fxl + (Fraction(float(py[y])) - fyl) * (fxh - fxl) / (fyh - fyl)
                e = ulps * ulp_of(max(abs(c), abs(c - fxl)))
                if c <= pxf[0]:
                    k = 0
                elif c > pxf[-1]:
                    k = W
                else:
                    k = min(max(int((float(c) - gt[0]) / gt[1] - 0.5), 0), W - 1)
                    while k > 0 and pxf[k - 1] >= c:
                        k -= 1
                    while k < W and pxf[k] < c:
                        k += 1
                toggle[y, k] += 1                                            # columns k.. have c <= px
                if e * 4 < Fraction(gt[1]):
                    for n in (k - 1, k):
                        if 0 <= n < W and abs(pxf[n] - c) <= e:
                            near[y, n] = True
                else:                                                        # E of a pixel's size: every one in reach
                    with np.errstate(all="ignore"):
                        near[y] |= np.abs(px - float(c)) <= 2.0 * float(e)
    inside = (np.cumsum(toggle, axis=1)[:, :W] & 1).astype(bool)
    return inside, near
