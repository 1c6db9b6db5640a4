"""GPU: the pair histogram per zone (gcn10_gpu_zonal_pair_histogram) through the ABI face, against numpy: per zone a
bincount over (bin of the soil code, landcover) of the pixels its spans name.  Shapes are the smallest at which the
kernel can go wrong: widths around the 16-pixel column group, a last row that ends off a group, spans of one pixel,
item boundaries inside a zone and inside a row, more zones than workgroups; and the spans of a real plan, a
tessellation read from a shapefile."""
import numpy as np
import pytest

from gcn10_amd import gpu, host
from tests import zoneutil
from tests.test_gpu_stats import model_histogram, soil_code
from tests.util import ESA_NASTY, HSG_NASTY

pytestmark = pytest.mark.gpu

HIST = 16 * 256
N_RANDOM = 1100             # more zones than the 4 workgroups per CU of a 256-CU device
BOUNDS = [(0, 0), (16, 48), (5, 7)]     # (max_span_px, max_item_px): the built-in ones and two small ones


class Scene:
    """Landcover, soil and index maps of a W x rows strip on the device, tile prepared; cj repeats and goes back."""

    def __init__(self, eng, W, rows, ratio, seed):
        rng = np.random.default_rng(seed)
        self.eng, self.W, self.rows = eng, W, rows
        small = rng.choice(ESA_NASTY, size=((rows + 5) // 6, (W + 8) // 9))
        esa = np.repeat(np.repeat(small, 6, axis=0), 9, axis=1)[:rows, :W]
        noise = rng.integers(0, 256, size=esa.shape)
        self.esa = np.ascontiguousarray(np.where(noise < 60, rng.choice(ESA_NASTY, size=esa.shape), esa).astype(np.uint8))
        hsx, hsy = W // ratio + 2, rows // ratio + 3
        self.coarse = rng.choice(HSG_NASTY, size=(hsy, hsx)).astype(np.uint8)
        gt = [0.0, 1.0 / W, 0.0, 1.0, 0.0, -1.0 / W]
        sgt = [-0.013, ratio / W, 0.0, 1.02, 0.0, -ratio / W]
        ci, cj = host.build_index_maps(gt, sgt, W, rows, hsx, hsy)
        cj = cj.copy()
        cj[rows // 2:] = cj[rows // 2:][::-1]               # decreasing
        cj[rows // 4:rows // 4 + 3] = cj[rows // 4]         # repeated
        self.ci, self.cj = ci, cj
        codes = gpu.pair_histogram_codes()
        lut = np.zeros(256, np.int64)
        for b in range(9):
            lut[codes[b]] = b
        soil = self.coarse[cj[:, None], ci[None, :]]
        self.key = lut[soil_code(soil)] * 256 + self.esa.astype(np.int64)       # [rows][W]
        self.soil = soil
        self.bufs = [eng.upload(a) for a in (self.esa, self.coarse, ci, cj)]
        eng.prepare_tile(self.bufs[1].ptr, hsx, hsy, self.bufs[2].ptr, W)

    def model(self, spans, n_zones):
        want = np.zeros((n_zones, HIST), np.uint64)
        for s in spans:
            np.add.at(want[s["zone"]], self.key[s["y"], s["x0"]:s["x1"]], 1)
        return want

    def run(self, spans, items, n_zones, hist=None, clear=True):
        own = hist is None
        hist = hist or self.eng.alloc(n_zones * HIST * 8)
        try:
            if clear:
                self.eng.memset(hist.ptr, 0, n_zones * HIST * 8)
            self.eng.zonal_pair_histogram(self.bufs[0].ptr, self.W, self.rows, self.bufs[3].ptr, spans, items, n_zones,
                                          hist.ptr)
            return self.eng.download(hist.ptr, (n_zones, HIST), np.uint64)
        finally:
            if own:
                hist.close()

    def close(self):
        for b in self.bufs:
            b.close()


def case_spans(W, rows, rng):
    """Zones 0..5 by hand (zone 3 has no span), then N_RANDOM zones of one random span each."""
    last = rows - 1
    sp = [(y, 0, W, 0) for y in range(rows)]                                    # 0: the whole strip, every row
    for y in (0, 7, last):                                                       # 1: spans of one pixel, x0 % 16 = 0, 1, 15
        sp += [(y, x, x + 1, 1) for x in sorted({0, 1, 15, 16, 17, 31, W - 1}) if 0 <= x < W]
    sp += [(last - 1, max(0, W - 5), W, 2), (last, max(0, W - 20), W, 2)]        # 2: ends at W, also on the LAST row
    z4 = [(3, 17, min(W, 22), 4), (5, 3, min(W, 45), 4), (9, 0, min(W, 6), 4), (9, min(W, 9), min(W, 40), 4),
          (10, 15, min(W, 17), 4)]                                               # 4: inside a group, across groups, two on a row
    sp += [s for s in z4 if s[1] < s[2]]
    z5 = [(5, 20, min(W, 60), 5), (9, 2, min(W, 12), 5), (last, 0, W, 5)]        # 5: shares pixels with 4, 2 and 0
    sp += [s for s in z5 if s[1] < s[2]]
    for k in range(N_RANDOM):
        y, x0 = int(rng.integers(0, rows)), int(rng.integers(0, W))
        sp.append((y, x0, min(W, x0 + 1 + int(rng.integers(0, 40))), 6 + k))
    a = np.array(sp, host.ZONE_SPAN_DTYPE)
    return a[np.lexsort((a["x0"], a["y"], a["zone"]))], 6 + N_RANDOM


@pytest.mark.parametrize("ratio", [25, 7])
@pytest.mark.parametrize("W", [1, 15, 16, 17, 33, 1047])
def test_zones_equal_numpy_counts_for_three_item_bounds(engine, W, ratio):
    rows = 48
    sc = Scene(engine, W, rows, ratio, seed=W * 100 + ratio)
    try:
        spans, n_zones = case_spans(W, rows, np.random.default_rng(W + ratio))
        want = sc.model(spans, n_zones)
        assert not want[3].any() and want[0].sum() == W * rows
        got = []
        for span_px, item_px in BOUNDS:
            s2, items = host.zone_items(spans, span_px, item_px)
            if (span_px, item_px) == (5, 7):
                # an item boundary inside zone 0 and, wherever the row is longer than an item, inside a row
                in_zone0 = items[s2["zone"][items["first_span"]] == 0]
                assert len(in_zone0) > 1
                if W > 7:
                    firsts = s2[in_zone0["first_span"]]
                    assert (firsts["x0"] > 0).any()
            got.append(sc.run(s2, items, n_zones))
        for g in got:
            np.testing.assert_array_equal(g, want)
    finally:
        sc.close()


def test_items_of_many_short_spans_equal_numpy_counts(engine):
    """Narrow zones give items of hundreds of spans: the prefix sum then runs over all four waves of the workgroup
    (65 to 255 spans), fills the 256 spans at hand exactly (256), and takes a second and a third pass over an item
    (257, 513, 700).  Each zone here is ONE item of mostly 1 to 3 px spans spread over the strip."""
    W, rows = 1047, 48
    counts = [700, 192, 256, 257, 64, 65, 513, 130, 255]
    sc = Scene(engine, W, rows, 25, seed=11)
    try:
        rng = np.random.default_rng(12)
        sp = []
        for zone, n in enumerate(counts):
            y = rng.integers(0, rows, n)
            x0 = rng.integers(0, W, n)
            length = np.where(rng.integers(0, 8, n) == 0, rng.integers(4, 60, n), rng.integers(1, 4, n))
            sp += [(int(a), int(b), int(min(W, b + c)), zone) for a, b, c in zip(y, x0, length)]
        a = np.array(sp, host.ZONE_SPAN_DTYPE)
        spans = a[np.lexsort((a["x0"], a["y"], a["zone"]))]
        want = sc.model(spans, len(counts))
        s2, items = host.zone_items(spans, 4096, 1 << 20)
        assert items["n_spans"].tolist() == counts                              # one item per zone, no span split
        np.testing.assert_array_equal(sc.run(s2, items, len(counts)), want)
        # the same spans as ONE zone in one item of 2432 spans, and under a bound that cuts the items short
        one = spans.copy()
        one["zone"] = 0
        one = one[np.lexsort((one["x0"], one["y"]))]
        s3, items3 = host.zone_items(one, 4096, 1 << 20)
        assert items3["n_spans"].tolist() == [sum(counts)]
        np.testing.assert_array_equal(sc.run(s3, items3, 1)[0], want.sum(axis=0))
        s4, items4 = host.zone_items(spans, 16, 600)
        assert 64 < int(items4["n_spans"].max()) < 256
        np.testing.assert_array_equal(sc.run(s4, items4, len(counts)), want)
    finally:
        sc.close()


@pytest.mark.parametrize("W,rows", [(1047, 48), (4096, 32)])
def test_one_zone_over_the_strip_equals_the_pair_histogram(engine, W, rows):
    sc = Scene(engine, W, rows, 25, seed=W)
    hist = engine.alloc(HIST * 8)
    try:
        engine.memset(hist.ptr, 0, HIST * 8)
        engine.pair_histogram(sc.bufs[0].ptr, W, rows, sc.bufs[3].ptr, hist.ptr)
        plain = engine.download(hist.ptr, (HIST,), np.uint64)
        np.testing.assert_array_equal(plain, model_histogram(sc.esa, sc.soil))
        whole = np.array([(y, 0, W, 0) for y in range(rows)], host.ZONE_SPAN_DTYPE)
        for span_px, item_px in BOUNDS:
            s2, items = host.zone_items(whole, span_px, item_px)
            np.testing.assert_array_equal(sc.run(s2, items, 1)[0], plain)       # bin for bin
    finally:
        hist.close()
        sc.close()


def test_a_tessellation_planned_from_a_shapefile_counts_its_hull_once(engine, tmp_path):
    """The kernel on a real plan: 1152 triangles with every vertex on a pixel centre (tests/test_zones_ties.py), read
    from a shapefile and scan-converted by gcn10_zones_build_plan.  Each zone against numpy over its spans, and all
    zones together, bin for bin, against the pair histogram of the rectangle the rule gives to the lattice's hull: a
    pixel on a shared edge counted twice or not at all shows here.  More zones than workgroups: zones change inside
    a workgroup."""
    W, rows = 203, 151
    gt = zoneutil.TIE_GTS[0]
    rings, (x0, x1, y0, y1) = zoneutil.lattice_triangles(gt, 1, 2, 24, 24, 8, 6, seed=5)
    zoneutil.write_zone_shapefile(str(tmp_path / "z"), [(i, [r]) for i, r in enumerate(rings)])
    sc = Scene(engine, W, rows, 7, seed=21)
    try:
        hull = model_histogram(sc.esa[y0:y1, x0:x1], sc.soil[y0:y1, x0:x1])
        assert int(hull.sum()) == (x1 - x0) * (y1 - y0) == 192 * 144
        with host.Zones(str(tmp_path / "z.shp")) as z:
            plans = [z.build_plan(gt, W, rows, max_span_px=s, max_item_px=i) for s, i in ((0, 0), (5, 7))]
        assert len(plans[1]["spans"]) > len(plans[0]["spans"]) and len(plans[1]["items"]) > len(plans[0]["items"])
        for plan in plans:
            n_zones = len(plan["local_zone"])
            assert n_zones == len(rings) == 1152
            want = sc.model(plan["spans"], n_zones)
            np.testing.assert_array_equal(want.sum(axis=1), plan["local_pixels"])
            got = sc.run(plan["spans"], plan["items"], n_zones)
            np.testing.assert_array_equal(got, want)
            np.testing.assert_array_equal(got.sum(axis=0), hull)
    finally:
        sc.close()


def test_two_calls_add_and_no_items_leave_the_histogram_alone(engine):
    W, rows = 33, 20
    sc = Scene(engine, W, rows, 7, seed=3)
    n_zones = 3
    hist = engine.alloc(n_zones * HIST * 8)
    try:
        a = np.array([(0, 0, 33, 0), (19, 30, 33, 0), (4, 5, 21, 2)], host.ZONE_SPAN_DTYPE)
        b = np.array([(19, 0, 33, 0), (4, 0, 33, 2), (5, 16, 32, 2)], host.ZONE_SPAN_DTYPE)
        one = sc.run(*host.zone_items(a), n_zones, hist=hist)
        np.testing.assert_array_equal(one, sc.model(a, n_zones))
        two = sc.run(*host.zone_items(b), n_zones, hist=hist, clear=False)
        np.testing.assert_array_equal(two, sc.model(a, n_zones) + sc.model(b, n_zones))
        assert not two[1].any()
        empty = np.zeros(0, host.ZONE_SPAN_DTYPE)
        three = sc.run(empty, np.zeros(0, host.ZONE_ITEM_DTYPE), n_zones, hist=hist, clear=False)
        np.testing.assert_array_equal(three, two)
    finally:
        hist.close()
        sc.close()


def test_the_face_checks_spans_and_items_before_upload(engine):
    W, rows = 33, 20
    sc = Scene(engine, W, rows, 7, seed=4)
    hist = engine.alloc(2 * HIST * 8)
    try:
        ok_items = np.array([(0, 1)], host.ZONE_ITEM_DTYPE)
        for bad in [(20, 0, 5, 0), (-1, 0, 5, 0), (3, 5, 5, 0), (3, 30, 34, 0), (3, -1, 4, 0), (3, 0, 4, 2), (3, 0, 4, -1)]:
            with pytest.raises(ValueError, match="span"):
                engine.zonal_pair_histogram(sc.bufs[0].ptr, W, rows, sc.bufs[3].ptr,
                                            np.array([bad], host.ZONE_SPAN_DTYPE), ok_items, 2, hist.ptr)
        two = np.array([(1, 0, 5, 0), (2, 0, 5, 1)], host.ZONE_SPAN_DTYPE)
        for items in [[(0, 2)], [(0, 1)], [(1, 1), (0, 1)], [(0, 1), (1, 2)], [(0, 0), (0, 1), (1, 1)]]:
            with pytest.raises(ValueError, match="items"):
                engine.zonal_pair_histogram(sc.bufs[0].ptr, W, rows, sc.bufs[3].ptr, two,
                                            np.array(items, host.ZONE_ITEM_DTYPE), 2, hist.ptr)
        # an unprepared width is refused as by gcn10_gpu_pair_histogram
        with pytest.raises(RuntimeError, match="prepare"):
            engine.zonal_pair_histogram(sc.bufs[0].ptr, 32, rows, sc.bufs[3].ptr,
                                        np.array([(1, 0, 5, 0)], host.ZONE_SPAN_DTYPE), ok_items, 2, hist.ptr)
    finally:
        hist.close()
        sc.close()
