"""CPU: the full-size checks' own parts (tests/fullblock.py) -- the table route of the reference against the
oracle's block pass, the banded overview model against itself unbanded, and the comparator's report of a wrong
pixel."""
import numpy as np
import pytest

from oracle import cn_oracle_c as oc
from tests import fullblock as fb
from tests.util import make_block, random_tables


@pytest.fixture(scope="module")
def T(tables):
    return fb.value_table(tables)


@pytest.mark.parametrize("seed,H,W,hsy,hsx", [(1, 300, 1040, 13, 43), (2, 257, 3, 12, 2), (3, 1, 36001, 2, 1441),
                                               (4, 700, 513, 29, 22)])
def test_table_route_equals_the_oracle(tables, T, seed, H, W, hsy, hsx):
    esa, gt, coarse, sgt = make_block(seed, H, W, hsy, hsx, nasty=True)
    want = oc.process_block_mem(esa, gt, coarse, sgt, tables)
    key = fb.block_keys(esa, gt, coarse, sgt)
    for r in range(18):
        np.testing.assert_array_equal(fb.expected_rows(T, key, r), want[r], err_msg="raster %d" % r)
    # a band of rows has the pairs of the same rows of the whole block
    np.testing.assert_array_equal(fb.block_keys(esa[H // 3:], [gt[0], gt[1], 0.0, gt[3] + (H // 3) * gt[5], 0.0, gt[5]],
                                                coarse, sgt), key[H // 3:])
    # the histogram route of the statistics
    khist = fb.key_histogram(key)
    for r in (0, 8, 9, 17):
        np.testing.assert_array_equal(fb.raster_histogram(T, khist, r), np.bincount(want[r].reshape(-1), minlength=256))


@pytest.mark.parametrize("cond_mask,table_mask", [(1, 0x1FF), (2, 0b100010001), (3, 0b10)])
def test_table_route_equals_the_oracle_on_subsets(tables, cond_mask, table_mask):
    t = random_tables(cond_mask * 1000 + table_mask)
    T = fb.value_table(t)
    esa, gt, coarse, sgt = make_block(11 + cond_mask, 130, 2049, 7, 83, nasty=True)
    want = oc.process_block_mem(esa, gt, coarse, sgt, t, cond_mask=cond_mask, table_mask=table_mask)
    key = fb.block_keys(esa, gt, coarse, sgt)
    for r in range(18):
        if (cond_mask >> (r // 9)) & 1 and (table_mask >> (r % 9)) & 1:
            np.testing.assert_array_equal(fb.expected_rows(T, key, r), want[r], err_msg="raster %d" % r)


@pytest.mark.parametrize("H,W,L,band", [(700, 1037, 2, 4), (513, 300, 2, 8), (2049, 70, 8, 256), (257, 3, 1, 2),
                                        (1500, 900, 3, 24)])
def test_banded_average_model_equals_one_band(H, W, L, band):
    rng = np.random.default_rng(H + W)
    full = rng.integers(0, 256, (H, W)).astype(np.uint8)
    full[rng.random((H, W)) < 0.3] = 255
    whole = fb.average_levels(full, L, band=1 << 30)
    banded = fb.average_levels(full, L, band=band)
    assert len(whole) == len(banded) == L
    for k in range(L):
        assert whole[k].shape == (-(-H // 2 ** (k + 1)), -(-W // 2 ** (k + 1)))
        np.testing.assert_array_equal(banded[k], whole[k], err_msg="level %d" % (k + 1))


def test_comparator_locates_the_first_wrong_pixel(tables, T):
    """One wrong pixel at the last row and column, on both sides of a strip boundary, and in raster 17: each is
    reported with its block, raster, row, column, values, strip and tile."""
    H, W = 2600, 700
    esa, gt, coarse, sgt = make_block(5, H, W, 20, 9, nasty=True)
    key = fb.block_keys(esa, gt, coarse, sgt)
    for r, y, x in [(0, H - 1, W - 1), (3, 2304, 0), (5, 2303, 511), (17, 1000, 257), (17, 0, 0)]:
        want = fb.expected_rows(T, key, r)
        got = want.copy()
        got[y, x] ^= 0x5A
        fb.compare(want, want, "A", r)                  # equal: nothing raised
        with pytest.raises(fb.Mismatch) as e:
            fb.compare(got, want, "A", r)
        m = e.value
        assert (m.block, m.raster, m.level, m.row, m.col) == ("A", r, 0, y, x)
        assert (m.got, m.want) == (int(got[y, x]), int(want[y, x]))
        assert m.strip == y // 2304 and m.tile == (y // 256, x // 256)
        assert "row %d col %d" % (y, x) in str(m) and "raster %d" % r in str(m)
        # a band of rows reports rows of the block, and the strip of the program's strip height
        with pytest.raises(fb.Mismatch) as e:
            fb.compare(got[y // 2:], want[y // 2:], "B", r, y0=y // 2, strip_rows=4096)
        assert (e.value.row, e.value.col, e.value.strip) == (y, x, y // 4096)
    # an overview level: rows of the level, the strip of its full-resolution rows
    lv = np.zeros((40, 30), np.uint8)
    bad = lv.copy()
    bad[39, 29] = 1
    with pytest.raises(fb.Mismatch) as e:
        fb.compare(bad, lv, "C", 9, y0=100, level=3)
    assert (e.value.level, e.value.row, e.value.col, e.value.strip) == (3, 139, 29, (139 << 3) // 2304)
    with pytest.raises(AssertionError, match="shape"):
        fb.compare(got[:-1], want, "A", 0)
