"""CPU: the GDAL tags of the writer (GDAL_NODATA 42113, GDAL_METADATA 42112) on plain files and COGs, and the host
half of the band statistics -- a raster's histogram from a pair histogram, GDAL's statistics of it, and the
GDAL_METADATA text -- against numpy statistics of the same pixels made by the numpy oracle."""
import math
import os
import zlib

import numpy as np
import pytest
from PIL import Image

from gcn10_amd import gpu, host
from oracle import cn_oracle_np as onp
from tests import cogcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GT = [10.0, 0.001, 0.0, 50.0, 0.0, -0.001]
LOOKUPS = os.path.join(ROOT, "tests", "golden", "lookups")
SOIL_CLASSES = np.array([0, 1, 2, 3, 4, 11, 12, 13, 14, 255, 5, 7, 10, 15], np.uint8)
LC_CLASSES = np.array([0, 10, 20, 30, 40, 50, 60, 70, 80, 90, 95, 100, 1, 33, 200, 255], np.uint8)


def soil_code(h):
    """soil_code() of gcn10_device_util.hpp: drained plane | undrained plane << 4, plane 5 = invalid."""
    h = np.asarray(h, np.int64)
    dual = (h >= 11) & (h <= 14)
    plain = np.where(h < 5, h, 5)
    d = np.where(dual, 4, plain)
    u = np.where(dual, h - 10, plain)
    return (d | (u << 4)).astype(np.uint8)


def expected_codes():
    codes = np.full(16, 0x55, np.uint8)
    for d in range(6):
        codes[d] = d | d << 4
    for u in range(1, 4):
        codes[5 + u] = 4 | u << 4
    return codes


def pair_histogram(esa, soil):
    """numpy model of gcn10_gpu_pair_histogram: [bin][landcover] counts."""
    codes = expected_codes()
    bin_of = {int(c): b for b, c in enumerate(codes) if b < 9}
    sc = soil_code(soil).reshape(-1)
    lut = np.zeros(256, np.int64)
    for c, b in bin_of.items():
        lut[c] = b
    bins = lut[sc]
    h = np.zeros(16 * 256, np.uint64)
    np.add.at(h, bins * 256 + esa.reshape(-1).astype(np.int64), 1)
    return h


def np_stats(v, nodata):
    v = np.asarray(v, np.float64).reshape(-1)
    valid = v if nodata is None else v[v != nodata]
    if valid.size == 0:
        return None
    return dict(min=valid.min(), max=valid.max(), mean=valid.mean(), stddev=valid.std(),
                valid_percent=100.0 * valid.size / v.size)


def check_stats(st, want):
    assert st["min"] == want["min"] and st["max"] == want["max"]
    assert st["mean"] == pytest.approx(want["mean"], rel=1e-12, abs=1e-12)
    assert st["stddev"] == pytest.approx(want["stddev"], rel=1e-12, abs=1e-9)
    assert st["valid_percent"] == pytest.approx(want["valid_percent"], rel=1e-12)


@pytest.fixture(scope="module")
def tables():
    return host.load_all_lookup_tables(LOOKUPS)


def test_bin_layout_is_the_gpu_librarys():
    np.testing.assert_array_equal(gpu.pair_histogram_codes(), expected_codes())


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("nodata", [None, 255, 0, 70])
def test_histogram_to_statistics_against_the_oracle(tables, seed, nodata):
    rng = np.random.default_rng(seed)
    H, W = 61, 83
    esa = rng.choice(LC_CLASSES, size=(H, W))
    soil = rng.choice(SOIL_CLASSES, size=(H, W))
    pair = pair_histogram(esa, soil)
    codes = gpu.pair_histogram_codes()
    for k in range(9):
        for drained in (True, False):
            want_px = onp.calculate_cn(esa, onp.modify_hysogs_data(soil, drained), tables[k])
            hist = host.raster_histogram(pair, codes, tables[k], drained)
            np.testing.assert_array_equal(hist, np.bincount(want_px.reshape(-1), minlength=256))
            st = host.band_stats(hist, nodata)
            want = np_stats(want_px, nodata)
            assert st["total"] == H * W
            if want is None:
                assert st["valid"] == 0 and st["xml"] is None
            else:
                check_stats(st, want)


def test_dual_classes_differ_between_conditions(tables):
    # every pixel a dual class: drained uses plane 4 (D), undrained planes 1..4
    esa = np.full((4, 4), 10, np.uint8)
    soil = np.array([[11, 12, 13, 14]] * 4, np.uint8)
    pair = pair_histogram(esa, soil)
    codes = gpu.pair_histogram_codes()
    k = 4
    hd = host.raster_histogram(pair, codes, tables[k], True)
    hu = host.raster_histogram(pair, codes, tables[k], False)
    assert hd[int(tables[k][10][4])] == 16
    assert not np.array_equal(hd, hu)
    want = onp.calculate_cn(esa, onp.modify_hysogs_data(soil, False), tables[k])
    np.testing.assert_array_equal(hu, np.bincount(want.reshape(-1), minlength=256))


def test_nodata_and_unknown_landcover_map_to_255(tables):
    # landcover 0 (NoData in the tables) and classes no table lists, on valid soil
    esa = np.array([[0, 1, 33, 200, 255]], np.uint8)
    soil = np.array([[1, 2, 3, 4, 1]], np.uint8)
    for k in range(9):
        hist = host.raster_histogram(pair_histogram(esa, soil), gpu.pair_histogram_codes(), tables[k], True)
        assert hist[255] == 5 and hist.sum() == 5
        st = host.band_stats(hist, 255)
        assert st["valid"] == 0 and st["xml"] is None       # all NoData: no items at all
        st = host.band_stats(hist, None)
        assert (st["min"], st["max"], st["valid_percent"]) == (255, 255, 100.0) and st["xml"] is not None


def test_counts_above_2_to_the_32(tables):
    rng = np.random.default_rng(7)
    esa = rng.choice(LC_CLASSES, size=(40, 50))
    soil = rng.choice(SOIL_CLASSES, size=(40, 50))
    pair = pair_histogram(esa, soil)
    big = (1 << 33) + 12345
    codes = gpu.pair_histogram_codes()
    for k in (0, 4, 8):
        px = onp.calculate_cn(esa, onp.modify_hysogs_data(soil, False), tables[k])
        hist = host.raster_histogram(pair * np.uint64(big), codes, tables[k], False)
        np.testing.assert_array_equal(hist, np.bincount(px.reshape(-1), minlength=256).astype(np.uint64) * np.uint64(big))
        for nodata in (None, 255):
            st = host.band_stats(hist, nodata)
            assert st["total"] == px.size * big
            check_stats(st, np_stats(px, nodata))       # scaling every count leaves the statistics as they are


def test_statistics_of_a_skewed_huge_histogram_are_exact():
    # one pixel of 0 among 2^40 pixels of 200: sums beyond 2^64 in v^2 terms need the 128-bit path
    hist = np.zeros(256, np.uint64)
    hist[200] = 1 << 40
    hist[0] = 1
    st = host.band_stats(hist)
    n = (1 << 40) + 1
    mean = 200.0 * (1 << 40) / n
    assert st["mean"] == mean
    assert st["stddev"] == pytest.approx(200.0 * math.sqrt(1 << 40) / n, rel=1e-12)


def test_metadata_text_format():
    hist = np.zeros(256, np.uint64)
    hist[[61, 98, 255]] = [3, 1, 4]
    st = host.band_stats(hist, 255)
    mean = (3 * 61 + 98) / 4
    std = math.sqrt((3 * 61 ** 2 + 98 ** 2) / 4 - mean ** 2)
    assert st["xml"] == (
        "<GDALMetadata>\n"
        '  <Item name="STATISTICS_MAXIMUM" sample="0">98</Item>\n'
        '  <Item name="STATISTICS_MEAN" sample="0">70.25</Item>\n'
        '  <Item name="STATISTICS_MINIMUM" sample="0">61</Item>\n'
        '  <Item name="STATISTICS_STDDEV" sample="0">%.14g</Item>\n'
        '  <Item name="STATISTICS_VALID_PERCENT" sample="0">50</Item>\n'
        "</GDALMetadata>\n" % std)
    assert "%.14g" % std == "16.021469970012"
    hist[[61, 98, 255]] = [1, 1, 1]
    assert 'VALID_PERCENT" sample="0">66.67<' in host.band_stats(hist, 255)["xml"]
    assert 'MEAN" sample="0">79.5<' in host.band_stats(hist, 255)["xml"]


# ---- the writer's tags --------------------------------------------------------------------------------------------

def tile_of(img, tx, ty):
    t = np.zeros((256, 256), np.uint8)
    part = img[ty * 256:(ty + 1) * 256, tx * 256:(tx + 1) * 256]
    t[:part.shape[0], :part.shape[1]] = part
    return t.tobytes()


def image(W, H, k=0):
    w, h = math.ceil(W / 2 ** k), math.ceil(H / 2 ** k)
    img = ((np.arange(w)[None, :] // 7 + np.arange(h)[:, None] // 5 + k * 13) % 97).astype(np.uint8)
    img[::3, ::4] = 255
    return img


def xml_of(img, nodata):
    return host.band_stats(np.bincount(img.reshape(-1), minlength=256), nodata)["xml"]


def write(path, W, H, cog, nodata=None, xml=None, reserve=False, early=True):
    L = host.cog_levels(W, H) if cog else None
    wr = host.TiffWriter(path, W, H, GT, n_levels=L)
    try:
        if early:
            if nodata is not None:
                assert wr.set_nodata(nodata) == 0
            if reserve:
                assert wr.reserve_metadata() == 0
        imgs = {}
        for k in (range(L, -1, -1) if cog else [0]):
            imgs[k] = img = image(W, H, k)
            across, down = wr.tiles(k)
            for ty in range(down):
                for tx in range(across):
                    assert wr.put_tile(tx, ty, zlib.compress(tile_of(img, tx, ty)), level=k) == 0
        if not early and nodata is not None:
            assert wr.set_nodata(nodata) == (-1 if cog else 0)
        if xml is not None:
            assert wr.set_metadata_xml(xml) == 0
        wr.finish()
    except BaseException:
        wr.abort()
        raise
    return L, imgs


def pil_tags(path):
    out = []
    with Image.open(path) as im:
        k = 0
        while True:
            try:
                im.seek(k)
            except EOFError:
                break
            out.append((dict(im.tag_v2), np.array(im)))
            k += 1
    return out


def tag_order(path):
    return [list(tags) for _p, _e, tags, _r in cogcheck.read_ifds(open(path, "rb").read())]


@pytest.mark.parametrize("W,H", [(600, 300), (257, 3), (1, 1)])
@pytest.mark.parametrize("early", [True, False])
def test_plain_file_with_nodata_and_statistics(tmp_path, W, H, early):
    path = str(tmp_path / "plain.tif")
    xml = xml_of(image(W, H), 255)
    write(path, W, H, cog=False, nodata=255, xml=xml, early=early)
    (tags, px), = pil_tags(path)
    np.testing.assert_array_equal(px, image(W, H))
    assert tags[42113] == "255"
    order, = tag_order(path)
    assert order == sorted(order)
    if xml is None:                     # the 1 x 1 raster is all NoData: no statistics, no tag
        assert (W, H) == (1, 1) and 42112 not in tags and order[-1] == 42113
    else:
        assert tags[42112] == xml
        assert order[-2:] == [42112, 42113]


@pytest.mark.parametrize("W,H", [(700, 513), (200, 256), (36001, 300)])
def test_cog_with_nodata_and_statistics(tmp_path, W, H):
    path = str(tmp_path / "cog.tif")
    xml = xml_of(image(W, H), 0)
    L, imgs = write(path, W, H, cog=True, nodata=0, xml=xml, reserve=True)
    ifds = cogcheck.check_cog(path, n_levels=L)
    levels = pil_tags(path)
    assert len(levels) == L + 1
    for k, (tags, px) in enumerate(levels):
        np.testing.assert_array_equal(px, imgs[k])
        assert tags[42113] == "0"                       # NoData on every IFD, as GDAL writes it
        assert (42112 in tags) == (k == 0)              # statistics on the full-resolution IFD only
    assert levels[0][0][42112] == xml
    for k, (_p, _e, tags, _r) in enumerate(ifds):
        assert list(tags) == sorted(tags)
        assert 42113 in tags


def test_cog_reserved_room_without_text_holds_an_empty_element(tmp_path):
    path = str(tmp_path / "cog.tif")
    write(path, 513, 300, cog=True, nodata=255, reserve=True)
    cogcheck.check_cog(path)
    tags, _px = pil_tags(path)[0]
    assert tags[42112] == "<GDALMetadata>\n</GDALMetadata>\n"


def test_cog_refuses_late_layout_changes(tmp_path):
    path = str(tmp_path / "cog.tif")
    W, H = 513, 300
    wr = host.TiffWriter(path, W, H, GT, n_levels=host.cog_levels(W, H))
    try:
        assert wr.set_metadata_xml("<GDALMetadata>\n</GDALMetadata>\n") == -1    # no room reserved
        assert wr.reserve_metadata(64) == 0
        assert wr.set_metadata_xml("x" * 64) == -1                              # longer than the room
        img = image(W, H, 2)
        assert wr.put_tile(0, 0, zlib.compress(tile_of(img, 0, 0)), level=2) == 0
        assert wr.set_nodata(255) == -1                                         # directories already placed
        assert wr.reserve_metadata(128) == -1
    finally:
        wr.abort()


def test_default_files_have_neither_tag(tmp_path):
    for cog in (False, True):
        path = str(tmp_path / ("c.tif" if cog else "p.tif"))
        write(path, 513, 300, cog=cog)
        for tags, _px in pil_tags(path):
            assert 42112 not in tags and 42113 not in tags
