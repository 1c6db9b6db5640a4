"""CPU: the zone reader and the scan conversion (gcn10_amd/csrc/host/zones.c): shapefiles of a writer of its own, the
spans against a numpy point-in-polygon over every pixel centre, ownership across two overlapping blocks, the items,
and a stand-alone program under AddressSanitizer + UBSan over truncated and corrupted files, a tessellation on pixel
centres and huge coordinates.  The fixtures here keep clear of pixel centres; tests/test_zones_ties.py holds the
scan conversion to the cases where a centre lies on an edge or a vertex."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from gcn10_amd import host
from tests import zoneutil
from tests.conftest import ROOT

W, H = 203, 151
GT = [12.3, 0.0125, 0.0, 48.7, 0.0, -0.0075]


def geo(pts):
    """pixel coordinates (u, v) of the window -> the window's geographic coordinates"""
    return [(GT[0] + u * GT[1], GT[3] + v * GT[5]) for u, v in pts]


TRIANGLE = [geo([(10.3, 5.2), (80.7, 20.9), (30.1, 90.4)])]
U_SHAPE = [geo([(100.2, 10.3), (115.6, 10.7), (115.9, 60.2), (140.3, 60.6), (140.1, 10.2), (160.7, 10.9), (160.4, 80.3),
                (100.6, 80.8)])]
HOLED = [geo([(20.3, 100.2), (90.6, 100.7), (90.2, 140.4), (20.8, 140.1)]),
         geo([(40.3, 110.2), (40.6, 130.7), (70.2, 130.4), (70.8, 110.1)])]
OVER_A = [geo([(120.3, 90.2), (170.6, 95.7), (165.2, 135.4), (125.8, 130.1)])]
OVER_B = [geo([(150.3, 100.2), (195.6, 105.7), (190.2, 145.4), (145.8, 140.1)])]
PARTLY = [geo([(180.3, -20.2), (230.6, -10.7), (220.2, 40.4), (175.8, 30.1)])]
OUTSIDE = [geo([(300.3, 10.2), (330.6, 10.7), (320.2, 40.4)])]
CORNERS = [geo([(5, 120), (15, 120), (15, 145), (5, 145)])]
TWO_PARTS = [geo([(60.2, 60.3), (75.7, 62.1), (66.4, 75.9)]), geo([(80.2, 70.3), (95.7, 72.1), (86.4, 85.9)])]
ZONES = [(11, TRIANGLE), (12, U_SHAPE), (13, HOLED), (14, OVER_A), (15, OVER_B), (16, PARTLY), (17, OUTSIDE),
         (12, CORNERS), (19, None), (20, TWO_PARTS)]           # id 12 twice: duplicates are allowed


@pytest.fixture(scope="module", params=[5, 15])
def shp(request, tmp_path_factory):
    base = str(tmp_path_factory.mktemp("zones%d" % request.param) / "zones")
    zoneutil.write_zone_shapefile(base, ZONES, shape_type=request.param)
    return base + ".shp"


def test_reader_returns_ids_boxes_and_rings(shp):
    with host.Zones(shp) as z:
        assert z.n == len(ZONES)
        assert z.ids.tolist() == [zid for zid, _r in ZONES]
        for i, (_id, rings) in enumerate(ZONES):
            if rings is None:
                assert z.n_rings(i) == 0 and not z.bbox[i].any()
                continue
            assert z.n_rings(i) == len(rings)
            pts = np.array([p for r in rings for p in r])
            np.testing.assert_array_equal(z.bbox[i], [pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max()])
            for got, want in zip(z.rings(i), rings):
                np.testing.assert_array_equal(got[:-1], np.array(want))
                np.testing.assert_array_equal(got[-1], got[0])          # the writer closes rings


def test_reader_refuses_a_polyline_by_record(tmp_path):
    line = struct.pack("<i4d2i", 3, 0, 0, 1, 1, 1, 2) + struct.pack("<i", 0) + struct.pack("<4d", 0, 0, 1, 1)
    zoneutil.write_zone_shapefile(str(tmp_path / "z"), [(1, TRIANGLE), (2, None), (3, TRIANGLE)], raw_records={2: line})
    with pytest.raises(host.HostError, match=r"record 3: shape type 3"):
        host.Zones(str(tmp_path / "z.shp"))


def test_reader_refuses_a_missing_id_field_and_takes_a_named_one(tmp_path):
    zoneutil.write_zone_shapefile(str(tmp_path / "z"), [(7, TRIANGLE)], id_field="HYBAS")
    with pytest.raises(host.HostError, match='no "ID" field'):
        host.Zones(str(tmp_path / "z.shp"))
    with pytest.raises(host.HostError, match="not numeric"):
        host.Zones(str(tmp_path / "z.shp"), "NAME")
    with host.Zones(str(tmp_path / "z.shp"), "hybas") as z:
        assert z.ids.tolist() == [7]


def test_reader_accepts_a_null_shape(tmp_path):
    zoneutil.write_zone_shapefile(str(tmp_path / "z"), [(5, None)])
    with host.Zones(str(tmp_path / "z.shp")) as z:
        assert z.n == 1 and z.n_rings(0) == 0
        plan = z.build_plan(GT, W, H)
    assert len(plan["local_zone"]) == 0 and len(plan["spans"]) == 0 and len(plan["items"]) == 0


@pytest.mark.parametrize("what", ["part offset", "point count", "record length"])
def test_reader_checks_counts_and_offsets(tmp_path, what):
    zoneutil.write_zone_shapefile(str(tmp_path / "z"), [(1, HOLED)])
    p = tmp_path / "z.shp"
    b = bytearray(p.read_bytes())
    if what == "part offset":
        b[108 + 44 + 4:108 + 44 + 8] = struct.pack("<i", 99)        # second part beyond the 10 points
    elif what == "point count":
        b[108 + 40:108 + 44] = struct.pack("<i", 1 << 20)
    else:
        b[104:108] = struct.pack(">i", 1 << 20)
    p.write_bytes(bytes(b))
    with pytest.raises(host.HostError, match="record 1"):
        host.Zones(str(p))


def test_a_wrong_box_in_the_record_header_loses_no_pixel(tmp_path):
    """The rows scanned for a zone come from the box of its points, not from the one the record header claims."""
    zoneutil.write_zone_shapefile(str(tmp_path / "z"), [(1, TRIANGLE)])
    p = tmp_path / "z.shp"
    b = bytearray(p.read_bytes())
    pts = np.array(TRIANGLE[0])
    small = [pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].min() + GT[1], pts[:, 1].min() + GT[1]]
    b[108 + 4:108 + 36] = struct.pack("<4d", *small)
    p.write_bytes(bytes(b))
    with host.Zones(str(p)) as z:
        np.testing.assert_array_equal(z.bbox[0], [pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max()])
        plan = z.build_plan(GT, W, H)
    np.testing.assert_array_equal(zoneutil.spans_to_mask(plan["spans"], 0, W, H), zoneutil.zone_mask(TRIANGLE, GT, W, H))


def _check_sorted(spans):
    key = list(zip(spans["zone"].tolist(), spans["y"].tolist(), spans["x0"].tolist()))
    assert key == sorted(key)
    assert (spans["x0"] < spans["x1"]).all()


def test_fixture_has_no_ties():
    """No pixel centre within 1e-6 px of a crossing: the comparison with numpy below is then free of rounding."""
    for _id, rings in ZONES:
        if rings is None:
            continue
        _m, margin = zoneutil.zone_mask(rings, GT, W, H, with_margin=True)
        assert margin > 1e-6, (_id, margin)


def test_spans_equal_numpy_membership_of_every_pixel(shp):
    with host.Zones(shp) as z:
        plan = z.build_plan(GT, W, H)
    spans = plan["spans"]
    _check_sorted(spans)
    local = plan["local_zone"].tolist()
    assert local == [0, 1, 2, 3, 4, 5, 7, 9]            # not the one outside, not the null shape
    n_two_spans = 0
    for li, zi in enumerate(local):
        want = zoneutil.zone_mask(ZONES[zi][1], GT, W, H)
        got = zoneutil.spans_to_mask(spans, li, W, H)
        np.testing.assert_array_equal(got, want, err_msg="zone record %d" % zi)
        assert int(plan["local_pixels"][li]) == int(want.sum()) > 0
        if zi == 1:
            rows, counts = np.unique(spans[spans["zone"] == li]["y"], return_counts=True)
            n_two_spans = int((counts == 2).sum())
    assert n_two_spans > 30                             # the "U" has two spans per row over its arms
    assert not zoneutil.zone_mask(OUTSIDE, GT, W, H).any()
    # the rectangle on pixel corners: exactly its 10 x 25 pixels
    got = zoneutil.spans_to_mask(spans, local.index(7), W, H)
    want = np.zeros((H, W), bool)
    want[120:145, 5:15] = True
    np.testing.assert_array_equal(got, want)


def test_two_overlapping_blocks_count_every_pixel_once(tmp_path):
    px = 8.3333333333330430e-05                         # the landcover's pixel: a 0.04 degree block is 481 px wide
    t = [10.0, px, 0.0, 50.0, 0.0, -px]
    RX, RY = 1000, 400
    boxes = [[10.0, 49.97, 10.04, 50.0], [10.04, 49.97, 10.08, 50.0]]
    wins = [host.raster_window(t, RX, RY, b) for b in boxes]
    assert wins[0][0] + wins[0][2] == wins[1][0] + 1    # the windows share one column
    ring = [[(10.0213, 49.9951), (10.0637, 49.9912), (10.0581, 49.9763), (10.0187, 49.9789)]]
    zoneutil.write_zone_shapefile(str(tmp_path / "z"), [(1, ring)])
    whole = zoneutil.zone_mask(ring, t, RX, RY)
    total = 0
    with host.Zones(str(tmp_path / "z.shp")) as z:
        for (xo, yo, w, h, gt), box in zip(wins, boxes):
            plan = z.build_plan(gt, w, h, own=box)
            assert plan["local_zone"].tolist() == [0]
            got = zoneutil.spans_to_mask(plan["spans"], 0, w, h)
            want = zoneutil.zone_mask(ring, gt, w, h) & zoneutil.own_mask(gt, w, h, box)
            np.testing.assert_array_equal(got, want)
            total += int(plan["local_pixels"][0])
            unowned = z.build_plan(gt, w, h)
            assert int(unowned["local_pixels"][0]) >= int(plan["local_pixels"][0])
        both = sum(int(z.build_plan(gt, w, h)["local_pixels"][0]) for (_x, _y, w, h, gt) in wins)
    assert total == int(whole.sum())
    assert both > total                                 # without ownership the shared column counts twice


@pytest.mark.parametrize("span_px,item_px", [(0, 0), (16, 40), (7, 7), (1, 1), (50, 1000)])
def test_items_are_of_one_zone_and_cover_all_spans_once(shp, span_px, item_px):
    with host.Zones(shp) as z:
        ref = z.build_plan(GT, W, H, max_span_px=1 << 20, max_item_px=1 << 30)
        plan = z.build_plan(GT, W, H, max_span_px=span_px, max_item_px=item_px)
    spans, items = plan["spans"], plan["items"]
    _check_sorted(spans)
    assert plan["local_zone"].tolist() == ref["local_zone"].tolist()
    np.testing.assert_array_equal(plan["local_pixels"], ref["local_pixels"])
    for li in range(len(plan["local_zone"])):       # splitting loses no pixel
        np.testing.assert_array_equal(zoneutil.spans_to_mask(spans, li, W, H), zoneutil.spans_to_mask(ref["spans"], li, W, H))
    span_bound, item_bound = (span_px or 16384), max(item_px or 65536, span_px or 16384)
    assert ((spans["x1"] - spans["x0"]) <= span_bound).all()
    if span_px and span_px < 50:
        assert len(spans) > len(ref["spans"])
    at = 0
    for it in items:
        assert int(it["first_span"]) == at and it["n_spans"] > 0
        mine = spans[at:at + int(it["n_spans"])]
        assert len(set(mine["zone"].tolist())) == 1
        assert int((mine["x1"] - mine["x0"]).sum()) <= item_bound
        at += int(it["n_spans"])
    assert at == len(spans)


def test_item_builder_alone_splits_a_long_span():
    spans = np.array([(0, 0, 100, 0), (1, 3, 4, 0), (1, 10, 75, 1)], host.ZONE_SPAN_DTYPE)
    out, items = host.zone_items(spans, 32, 64)
    assert out.tolist() == [(0, 0, 32, 0), (0, 32, 64, 0), (0, 64, 96, 0), (0, 96, 100, 0), (1, 3, 4, 0),
                            (1, 10, 42, 1), (1, 42, 74, 1), (1, 74, 75, 1)]
    assert items.tolist() == [(0, 2), (2, 3), (5, 2), (7, 1)]
    with pytest.raises(host.HostError):
        host.zone_items(np.array([(0, 5, 5, 0)], host.ZONE_SPAN_DTYPE))


# ---- the reader and the scan conversion on damaged files, under AddressSanitizer + UBSan -----------------------------

def test_sanitized_program_survives_truncated_and_corrupted_files(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    exe = str(tmp_path / "zones_san")
    # both runtimes linked statically: the program then runs in any environment, whatever else is loaded before it
    cmd = [cc, "-std=c99", "-D_GNU_SOURCE", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-static-libasan", "-static-libubsan",
           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
           "-o", exe, os.path.join(ROOT, "tests", "zones_san_main.c"),
           os.path.join(ROOT, "gcn10_amd", "csrc", "host", "zones.c"), "-lm"]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(path):
        p = subprocess.run([exe, path, "%r" % GT[0], "%r" % GT[1], "%r" % GT[3], "%r" % GT[5], str(W), str(H)],
                           capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode in (0, 1), (path, p.returncode, p.stderr[-3000:])
        assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
        return p

    good = {}
    for st in (5, 15):
        base = str(tmp_path / ("z%d" % st))
        zoneutil.write_zone_shapefile(base, ZONES, shape_type=st)
        p = run(base + ".shp")
        assert p.returncode == 0 and p.stdout.startswith("zones %d local 8 " % len(ZONES)), p.stdout + p.stderr
        good[st] = base
    # ties: a tessellation with every vertex on a pixel centre, which owns each pixel of its hull once; and huge
    # coordinates: boxes around the window and triangles with one vertex up to 1.7e308 away, above, below and beside it
    rings, (x0, x1, y0, y1) = zoneutil.lattice_triangles(GT, 1, 2, 24, 24, 8, 6, seed=5)
    zoneutil.write_zone_shapefile(str(tmp_path / "ties"), [(i, [r]) for i, r in enumerate(rings)])
    p = run(str(tmp_path / "ties.shp"))
    assert p.returncode == 0 and p.stdout.startswith("zones 1152 local 1152 "), p.stdout + p.stderr
    assert p.stdout.split()[-2:] == ["pixels", str((x1 - x0) * (y1 - y0))], p.stdout
    far, near = [], [zoneutil.pt(GT, 20, 130), zoneutil.pt(GT, 60, 20)]
    for d in (1e6, 1e150, 1.7e308):
        far += [[[(-d, -d), (d, -d), (d, d), (-d, d)]], [near + [(d, d)]], [near + [(d, -d)]], [near + [(-d, near[0][1])]]]
    zoneutil.write_zone_shapefile(str(tmp_path / "far"), [(i, r) for i, r in enumerate(far)])
    p = run(str(tmp_path / "far.shp"))
    with np.errstate(all="ignore"):
        pixels = sum(int(zoneutil.zone_mask(r, GT, W, H).sum()) for r in far)
    assert p.returncode == 0 and p.stdout.startswith("zones %d local " % len(far)), p.stdout + p.stderr
    assert p.stdout.split()[-2:] == ["pixels", str(pixels)] and pixels >= 3 * W * H, p.stdout
    # every truncation and a few hundred single-byte corruptions of the Polygon file, in one run of the program
    # (it takes a directory and goes through its .shp files)
    shp = open(good[5] + ".shp", "rb").read()
    dbf = open(good[5] + ".dbf", "rb").read()
    d = tmp_path / "damaged"
    d.mkdir()
    n = 0

    def put(shp_bytes, dbf_bytes):
        nonlocal n
        (d / ("c%05d.shp" % n)).write_bytes(shp_bytes)
        (d / ("c%05d.dbf" % n)).write_bytes(dbf_bytes)
        n += 1

    for cut in range(len(shp)):
        put(shp[:cut], dbf)
    for cut in range(0, len(dbf), 3):
        put(shp, dbf[:cut])
    rng = np.random.default_rng(7)
    for _ in range(400):
        b = bytearray(shp)
        b[int(rng.integers(24, len(shp)))] = int(rng.integers(0, 256))
        put(bytes(b), dbf)
    for at in list(range(100, 160)) + list(range(108 + 36, 108 + 52)):      # record header, counts, first part offsets
        for v in (0x00, 0x7f, 0x80, 0xff):
            b = bytearray(shp)
            b[at] = v
            put(bytes(b), dbf)
    for _ in range(100):
        b = bytearray(dbf)
        b[int(rng.integers(0, len(dbf)))] = int(rng.integers(0, 256))
        put(shp, bytes(b))
    p = run(str(d))
    assert ("files %d " % n) in p.stdout, p.stdout[-500:]
