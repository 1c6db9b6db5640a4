"""CPU: the scan conversion (gcn10_amd/csrc/host/zones.c) where a pixel centre lies ON an edge or a vertex, which
tests/test_zones_host.py steps around.  Zones that tile an area own every pixel of it exactly once; the spans do not
depend on where a ring starts or which way it runs; the plan equals the numpy rule of tests/zoneutil.py and, where one
exists, a closed form; and away from the rounding of a crossing it equals even-odd membership in exact arithmetic.
Three geotransforms throughout (zoneutil.TIE_GTS)."""
import numpy as np
import pytest

from gcn10_amd import host
from tests import zoneutil
from tests.zoneutil import TIE_GTS, on_centres, pt

W, H = 203, 151
GT_IDS = ["plain", "landcover", "antimeridian"]


def _plan(tmp_path, zones, gt, w, h, raw_records=None, **kw):
    zoneutil.write_zone_shapefile(str(tmp_path / "z"), zones, raw_records=raw_records)
    with host.Zones(str(tmp_path / "z.shp")) as z:
        return z.build_plan(gt, w, h, **kw)


# ---- 1. two zones, one shared edge through pixel centres -------------------------------------------------------------

# Per geotransform: the window, and the least numbers of pairs kept of the 300 draws and of pairs whose two ring-order
# evaluations of the unoriented formula x1 + (py - y1) * (x2 - x1) / (y2 - y1) differ at some row v1+1 .. v2.  Measured
# with numpy: 173, 238 and 238 pairs kept; 32, 36 and 19 that differ.  The first two geotransforms are held to 30; the
# third's count was taken before its bound was set, which is the measured 19 less a margin of 2.
SHARED_EDGE = [(203, 151, 150, 30), (400, 400, 150, 30), (400, 400, 150, 17)]


def shared_edge_pairs(w, h):
    rng = np.random.default_rng(1)
    pairs = []
    for _ in range(300):
        u1, v1, k = int(rng.integers(0, w)), int(rng.integers(0, h)), int(rng.integers(1, 40))
        dx, dy = int(rng.integers(-3, 4)), int(rng.integers(1, 4))
        u2, v2 = u1 + k * dx, v1 + k * dy
        if 0 <= u2 < w and 0 <= v2 < h:
            pairs.append((u1, v1, u2, v2))
    return pairs


@pytest.mark.parametrize("case", range(3), ids=GT_IDS)
def test_two_zones_with_a_shared_edge_through_centres_share_no_pixel(tmp_path, case):
    gt = TIE_GTS[case]
    w, h, min_kept, min_differ = SHARED_EDGE[case]
    pairs = shared_edge_pairs(w, h)
    _px, py = zoneutil.centres(gt, w, h)
    xl, xr = gt[0] - gt[1], gt[0] + (w + 1) * gt[1]       # one pixel left and right of the window
    zones, differ = [], 0
    for u1, v1, u2, v2 in pairs:
        P, Q = pt(gt, u1, v1), pt(gt, u2, v2)
        zones.append((1, [[(xl, P[1]), P, Q, (xl, Q[1])]]))
        zones.append((2, [[(xr, Q[1]), Q, P, (xr, P[1])]]))
        rows = py[v1 + 1:v2 + 1]
        pq = P[0] + (rows - P[1]) * (Q[0] - P[0]) / (Q[1] - P[1])
        qp = Q[0] + (rows - Q[1]) * (P[0] - Q[0]) / (P[1] - Q[1])
        differ += bool((pq != qp).any())
    print("%d pairs kept, %d with two different evaluations of the unoriented crossing" % (len(pairs), differ))
    assert len(pairs) >= min_kept and differ >= min_differ          # the sweep means something
    plan = _plan(tmp_path, zones, gt, w, h)
    per_record = zoneutil.spans_by_record(plan, len(zones))
    pixels = np.zeros(len(zones), np.int64)
    pixels[plan["local_zone"]] = plan["local_pixels"].astype(np.int64)
    neither = both = 0
    bad = []
    for i, (u1, v1, u2, v2) in enumerate(pairs):
        cov = zoneutil.coverage(np.concatenate(per_record[2 * i:2 * i + 2]), w, h)
        assert not cov[:v1 + 1].any() and not cov[v2 + 1:].any()
        part = cov[v1 + 1:v2 + 1]
        if (part != 1).any() or pixels[2 * i] + pixels[2 * i + 1] != w * (v2 - v1):
            bad.append((u1, v1, u2, v2))
        neither += int((part == 0).sum())
        both += int((part > 1).sum())
    print("%d pairs: %d pixels in neither zone, %d in both; first failing pairs %s"
          % (len(pairs), neither, both, bad[:3]))
    assert (neither, both, bad) == (0, 0, [])


# ---- 2. a triangulated lattice owns every pixel of its hull exactly once ---------------------------------------------

LATTICES = [(1, 2, 24, 24, 8, 6), (3, 2, 28, 29, 7, 5)]        # u0, v0, cells across and down, their size in pixels


@pytest.mark.parametrize("lattice", LATTICES, ids=["8x6", "7x5"])
@pytest.mark.parametrize("gt", TIE_GTS, ids=GT_IDS)
def test_a_tessellation_covers_its_hull_exactly_once(tmp_path, gt, lattice):
    rings, (x0, x1, y0, y1) = zoneutil.lattice_triangles(gt, *lattice, seed=5)
    zones = [(i, [r]) for i, r in enumerate(rings)]
    assert len(zones) == 2 * lattice[2] * lattice[3] >= 1150
    want = np.zeros((H, W), np.int32)
    want[y0:y1, x0:x1] = 1
    np.testing.assert_array_equal(zoneutil.hull_mask(gt, W, H, rings), want.astype(bool))   # the index set is the rule's
    # an own box with all four sides on pixel centres: px == own[0] and py == own[3] are in, px == own[2] and
    # py == own[1] are out
    own = [pt(gt, 40, 0)[0], pt(gt, 0, 120)[1], pt(gt, 170, 0)[0], pt(gt, 0, 30)[1]]
    owned = np.zeros((H, W), bool)
    owned[30:120, 40:170] = True
    np.testing.assert_array_equal(zoneutil.own_mask(gt, W, H, own), owned)
    zoneutil.write_zone_shapefile(str(tmp_path / "z"), zones)
    with host.Zones(str(tmp_path / "z.shp")) as z:
        plan = z.build_plan(gt, W, H)
        cut = z.build_plan(gt, W, H, own=own)
    np.testing.assert_array_equal(zoneutil.coverage(plan["spans"], W, H), want)
    assert int(plan["local_pixels"].sum()) == (x1 - x0) * (y1 - y0)
    assert len(plan["local_zone"]) == len(zones)
    np.testing.assert_array_equal(zoneutil.coverage(cut["spans"], W, H), want * owned)
    assert int(cut["local_pixels"].sum()) == int((want * owned).sum()) == 90 * 130


@pytest.mark.parametrize("gt", TIE_GTS, ids=GT_IDS)
def test_a_tessellation_over_two_blocks_counts_every_pixel_once(tmp_path, gt):
    """Two blocks whose windows share a column, their common side ON that column's centres.  The rule speaks of a
    block's own centres, and a block's clipped geotransform (gt[0] = t[0] + xoff * t[1], as the reference forms it)
    gives centres that differ from the whole raster's by an ulp at some columns: there a side on the raster's centre is no
    tie for the block, and the blocks' totals need not be the raster's.  So every block is held to the rule on ITS
    centres, and the totals to the single window's at a common column (83) where the second block's centres equal the
    raster's on the common side and on the hull's sides under all three geotransforms -- asserted.  (At column 104
    they are an ulp off under two of the three.)"""
    RX, RY = 203, 151
    rings, (x0, x1, y0, y1) = zoneutil.lattice_triangles(gt, *LATTICES[0], seed=6)
    zones = [(i, [r]) for i, r in enumerate(rings)]
    side = pt(gt, 83, 0)[0]
    top, bottom = gt[3], gt[3] + RY * gt[5]
    boxes = [[gt[0], bottom, side, top], [side, bottom, gt[0] + RX * gt[1], top]]
    wins = [host.raster_window(gt, RX, RY, b) for b in boxes]
    assert wins[0][0] + wins[0][2] == wins[1][0] + 1 == 84             # the windows share column 83
    gpx, _gpy = zoneutil.centres(gt, RX, RY)
    zoneutil.write_zone_shapefile(str(tmp_path / "z"), zones)
    total = both = 0
    with host.Zones(str(tmp_path / "z.shp")) as z:
        single = z.build_plan(gt, RX, RY)
        for (xo, yo, w, h, bgt), box in zip(wins, boxes):
            assert yo == 0 and h == RY
            bpx, _bpy = zoneutil.centres(bgt, w, h)
            for col in (x0, x1, 83):                                   # the hull's sides and the common side
                if xo <= col < xo + w:
                    assert bpx[col - xo] == gpx[col]
            plan = z.build_plan(bgt, w, h, own=box)
            want = zoneutil.hull_mask(bgt, w, h, rings) & zoneutil.own_mask(bgt, w, h, box)
            np.testing.assert_array_equal(zoneutil.coverage(plan["spans"], w, h), want.astype(np.int32))
            total += int(plan["local_pixels"].sum())
            both += int(z.build_plan(bgt, w, h)["local_pixels"].sum())
    assert total == int(single["local_pixels"].sum()) == (x1 - x0) * (y1 - y0)
    assert both == total + (y1 - y0)                                   # without ownership column 83 counts twice


# ---- 3 to 5. fixtures with exact ties --------------------------------------------------------------------------------

def comb(gt, teeth, u0=10, top=20, mid=30, bottom=50):
    """A bar with `teeth` slanted teeth below it, 4 px wide every 8 px, vertices on centres: a row through the teeth
    has 2 * teeth crossings."""
    right = u0 + 8 * (teeth - 1) + 4
    uv = [(u0, top), (right, top)]
    for t in range(teeth - 1, -1, -1):
        u = u0 + 8 * t
        uv += [(u + 4, mid), (u + 6, bottom), (u + 2, bottom), (u, mid)]
    return [on_centres(gt, uv)]


def box_mask(x0, x1, y0, y1):
    m = np.zeros((H, W), bool)
    m[y0:y1, x0:x1] = True
    return m


def fixtures(gt):
    """(name, rings, closed form or None).  A closed form is (mask, where): the plan must equal mask on the pixels of
    where (None: on all).  Every vertex is a centre double, the far-away ones apart."""
    out = []

    def c(uv):
        return on_centres(gt, uv)

    def add(name, rings, closed=None):
        out.append((name, rings, closed))

    # columns [x0, x1) and the rows with y_lo <= py < y_hi: the top side's row is out, the bottom side's in
    add("rectangle on centre lines", [c([(20, 30), (60, 30), (60, 80), (20, 80)])], (box_mask(20, 60, 31, 81), None))
    nothing = np.zeros((H, W), bool)
    # a top vertex is crossed by neither of its edges; a bottom one by both, at the same x: its pixel is out both times
    add("vertex a local top", [c([(100, 20), (120, 50), (80, 50)])], (nothing, box_mask(0, W, 0, 21)))
    add("vertex a local bottom", [c([(80, 60), (120, 60), (100, 90)])], (nothing, box_mask(0, W, 90, H)))
    # a vertex the outline passes through is crossed by its upper edge alone, exactly at the vertex
    add("vertices passed through, left and right", [c([(100, 100), (130, 120), (110, 140), (90, 120)])],
        (box_mask(90, 130, 120, 121), box_mask(0, W, 120, 121)))
    # a trapezoid: the row of its top side is out, that of its bottom side in, from vertex to vertex
    add("horizontal edges on centre rows", [c([(30, 10), (70, 10), (80, 25), (20, 25)])],
        (box_mask(20, 80, 25, 26), box_mask(0, W, 0, 11) | box_mask(0, W, 25, H)))
    # A-B and C-D cross on the centre of (50, 110); off the two diagonals the two triangles are plain
    v, u = np.mgrid[0:H, 0:W]
    k = v - 100
    lo, hi = np.minimum(40 + k, 60 - k), np.maximum(40 + k, 60 - k)
    bow = (v > 100) & (v <= 120) & (((u >= 40) & (u < lo)) | ((u >= hi) & (u < 60)))
    add("bow-tie crossing on a centre", [c([(40, 100), (60, 120), (60, 100), (40, 120)])],
        (bow, (u != 40 + k) & (u != 60 - k)))
    add("spike", [c([(100, 40), (120, 40), (120, 60), (110, 60), (125, 75), (110, 60), (100, 60)])],
        (box_mask(100, 120, 41, 61), None))
    tri = [(10, 5), (80, 20), (30, 90)]
    add("consecutive duplicate points", [c([tri[0], tri[0], tri[1], tri[1], tri[1], tri[2]])],
        (zoneutil.zone_mask([c(tri)], gt, W, H), None))
    add("ring of one point", [c([(50, 50)])], (nothing, None))
    add("ring of two points", [c([(50, 50), (70, 80)])], (nothing, None))
    add("zero-area ring", [c([(50, 50), (70, 80), (90, 95), (70, 80)])], (nothing, None))
    # the shared edge (40,140)-(20,120) cancels under even-odd: what is left is one ring around the shell less the hole
    add("hole sharing an edge with its shell",
        [c([(20, 100), (90, 100), (90, 140), (40, 140), (20, 120)]), c([(20, 120), (40, 140), (50, 115)])],
        (zoneutil.zone_mask([c([(20, 100), (90, 100), (90, 140), (40, 140), (50, 115), (20, 120)])], gt, W, H), None))
    add("hole sharing a vertex with its shell",
        [c([(100, 100), (180, 100), (180, 145), (100, 145)]), c([(100, 145), (130, 120), (140, 135)])])
    add("two parts sharing an edge", [c([(150, 10), (190, 10), (150, 50)]), c([(190, 10), (190, 50), (150, 50)])],
        (box_mask(150, 190, 11, 51), None))
    for teeth in (8, 9, 20):                # 16 and 18 crossings: both sides of scan_zone's switch of sorts; and 40
        add("comb of %d teeth" % teeth, comb(gt, teeth))
    everything = (np.ones((H, W), bool), None)
    for d in (1e6, 1e150, 1.7e308):
        add("box %g away" % d, [[(-d, -d), (d, -d), (d, d), (-d, d)]], everything)
        add("triangle with a vertex %g away" % d, [[pt(gt, 20, 130), pt(gt, 60, 20), (d, d)]])
    return out


def far_lower_vertices(gt):
    """Triangles whose far vertex is a LOWER endpoint, below or beside the window: its edges' crossings are formed as
    far + (a difference of the far magnitude), which leaves no digit at the scale of a pixel.  Plan and rule must still
    agree to the bit and ring order must still not matter; exact arithmetic has nothing to say about them."""
    out = []
    for d in (1e6, 1e150, 1.7e308):
        out.append(("triangle with a lower vertex %g away, below" % d, [[pt(gt, 20, 130), pt(gt, 60, 20), (d, -d)]], None))
        out.append(("triangle with a lower vertex %g away, beside" % d,
                    [[pt(gt, 20, 130), pt(gt, 60, 20), (-d, pt(gt, 0, 140)[1])]], None))
    return out


def random_polygons(gt):
    """40 polygons of 3 to 8 vertices on pixel centres (self-crossing as they come)"""
    rng = np.random.default_rng(3)
    return [("random %d" % i, [on_centres(gt, [(int(rng.integers(5, W - 5)), int(rng.integers(5, H - 5)))
                                               for _ in range(int(rng.integers(3, 9)))])], None) for i in range(40)]


def crossings_in_row(spans, y):
    return 2 * int((spans["y"] == y).sum())


@pytest.mark.parametrize("gt", TIE_GTS, ids=GT_IDS)
def test_the_plan_equals_the_rule_and_the_closed_forms_at_ties(tmp_path, gt):
    fx = fixtures(gt) + far_lower_vertices(gt)
    px, py = zoneutil.centres(gt, W, H)
    for name, rings, _closed in fx:
        # exact ties: every vertex a centre double, or a crossing ON a centre (the far-away ones have none to show)
        on = [p[0] in px and p[1] in py for r in rings for p in r]
        with np.errstate(all="ignore"):
            margin = zoneutil.zone_mask(rings, gt, W, H, with_margin=True)[1]
        assert all(on) or margin == 0 or "away" in name, name
    plan = _plan(tmp_path, [(i, f[1]) for i, f in enumerate(fx)], gt, W, H)
    per_record = zoneutil.spans_by_record(plan, len(fx))
    local = plan["local_zone"].tolist()
    for i, (name, rings, closed) in enumerate(fx):
        with np.errstate(all="ignore"):
            want = zoneutil.zone_mask(rings, gt, W, H)
        got = zoneutil.coverage(per_record[i], W, H)
        np.testing.assert_array_equal(got, want.astype(np.int32), err_msg=name)
        assert (i in local) == bool(want.any()), name
        if i in local:
            assert int(plan["local_pixels"][local.index(i)]) == int(want.sum()), name
        if closed is not None:
            mask, where = closed
            where = np.ones((H, W), bool) if where is None else where
            np.testing.assert_array_equal(got.astype(bool)[where], mask[where], err_msg=name + " (closed form)")
    names = [f[0] for f in fx]
    for n in ("ring of one point", "ring of two points", "zero-area ring"):
        assert names.index(n) not in local
    for teeth in (8, 9, 20):                # a row through the teeth: one span per tooth
        assert crossings_in_row(per_record[names.index("comb of %d teeth" % teeth)], 40) == 2 * teeth


def test_an_open_ring_equals_the_closed_one(tmp_path):
    gt = TIE_GTS[0]
    ring = on_centres(gt, [(20, 100), (90, 100), (90, 140), (40, 140), (20, 120)])
    hole = on_centres(gt, [(30, 110), (40, 130), (60, 115)])
    raw = zoneutil.polygon_record([ring, hole])                  # neither ring repeats its first point
    plan = _plan(tmp_path, [(1, [ring, hole]), (2, None)], gt, W, H, raw_records={1: raw})
    with host.Zones(str(tmp_path / "z.shp")) as z:
        assert [len(r) for r in z.rings(0)] == [6, 4] and [len(r) for r in z.rings(1)] == [5, 3]
    a, b = zoneutil.spans_by_record(plan, 2)
    assert len(a) > 0
    np.testing.assert_array_equal(a[["y", "x0", "x1"]], b[["y", "x0", "x1"]])
    np.testing.assert_array_equal(zoneutil.coverage(b, W, H), zoneutil.zone_mask([ring, hole], gt, W, H).astype(np.int32))


@pytest.mark.parametrize("gt", TIE_GTS, ids=GT_IDS)
def test_ring_order_does_not_matter(tmp_path, gt):
    """The ring as given, reversed, and started at every other vertex: identical spans."""
    fx = fixtures(gt) + far_lower_vertices(gt) + random_polygons(gt)
    zones, first = [], []
    for _name, rings, _c in fx:
        first.append(len(zones))
        for k in range(max(len(r) for r in rings)):
            turned = [r[k % len(r):] + r[:k % len(r)] for r in rings]
            zones.append((len(zones), turned))
            zones.append((len(zones), [r[::-1] for r in turned]))
    first.append(len(zones))
    plan = _plan(tmp_path, zones, gt, W, H)
    per_record = zoneutil.spans_by_record(plan, len(zones))
    n_checked = 0
    for i, (name, _rings, _c) in enumerate(fx):
        ref = per_record[first[i]][["y", "x0", "x1"]]
        for j in range(first[i] + 1, first[i + 1]):
            np.testing.assert_array_equal(per_record[j][["y", "x0", "x1"]], ref,
                                          err_msg="%s, variant %d" % (name, j - first[i]))
            n_checked += 1
    assert n_checked == len(zones) - len(fx) > 700


# E of the exact comparison, in ulps of the largest magnitude of a crossing's expression; derived in the test below
E_ULPS = 7


@pytest.mark.parametrize("gt", TIE_GTS, ids=GT_IDS)
def test_the_plan_equals_exact_even_odd_membership_away_from_the_roundings(tmp_path, gt):
    """Against fractions.Fraction on the very doubles (centres as the rule computes them, vertices as stored).

    Which rows an edge crosses is decided by comparisons of doubles, which are exact.  The crossing is
        xc = xl + (py - yl) * (xh - xl) / (yh - yl)
    with five roundings in t = (py - yl) * (xh - xl) / (yh - yl) (two differences, a product, a quotient: four; the
    third difference makes five) and one in the sum.  With u = 2^-53 and without overflow or underflow,
        fl(t) = t (1 + d),  |d| <= (1 + u)^5 - 1 < 5.01 u,      fl(xc) = (xl + fl(t)) (1 + e),  |e| <= u,
    so |fl(xc) - xc| <= 5.01 u |t| (1 + u) + u |xc| < 6.02 u m with m = max(|t|, |xc|), where t = xc - xl is the exact
    one and |t| <= |xh - xl| because yl <= py < yh.  A double f has ulp(f) > u f, and the double f nearest to m has
    f >= m (1 - u), so 7 ulp(f) > 7 u m (1 - u) > 6.02 u m: E = 7 ulp(max(|xc|, |xc - xl|)), the largest magnitude the
    crossing's expression meets, bounds the error of that crossing.  (The far-away fixtures stay clear of overflow:
    their far vertex is an upper endpoint, so t stays small, and the box's far edges are vertical, t = 0.)  A pixel
    farther than E from every crossing of its row stands on the same side of each computed crossing as of the exact
    one, so its membership must be the exact one.  The pixels within E are excluded: fewer than 1 % of every fixture's
    pixels, asserted (measured: at most 0.53 %, the 161 of 30653 that lie on the far triangles' two near edges)."""
    fx = fixtures(gt) + random_polygons(gt)
    plan = _plan(tmp_path, [(i, f[1]) for i, f in enumerate(fx)], gt, W, H)
    per_record = zoneutil.spans_by_record(plan, len(fx))
    worst = 0.0
    for i, (name, rings, _c) in enumerate(fx):
        inside, near = zoneutil.exact_membership(rings, gt, W, H, E_ULPS)
        share = float(near.mean())
        worst = max(worst, share)
        assert share < 0.01, (name, share)
        got = zoneutil.coverage(per_record[i], W, H).astype(bool)
        np.testing.assert_array_equal(got[~near], inside[~near], err_msg=name)
    print("largest share of pixels within E of a crossing: %.4f %%" % (100.0 * worst))
