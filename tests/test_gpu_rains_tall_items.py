"""GPU: gcn10_gpu_grid_sums_rains in items taller than the launch's floor of 16 rows, up to the full 512 x 127 pixels
that every item of a block-sized call has.  The strips of tests/test_gpu_grid_rains.py are all short enough to stay at
the floor; this file runs the band arithmetic above it -- the shapes, the landcover and the closed forms are those of
tests/test_gpu_capped_grids.py ("6. grid_sums_rain"), imported, since the launch is the same one.

  - bands of 17 and 127 rows and the clamp to 127 on the 17-column strip, k = 2, against the summed oracle
    (tests/rainsutil.py);
  - the 528-column strip of full items, k = 3, the layers' bytes drawn from the three tables of full_item_tables: word
    2 + j against full_item_triples with field j.  That is the bin counted 65 024 times, the one counted 32 768 times,
    and a 32-bit layer sum of 65 024 x 65 535 in a piece and in the wave's total.
"""
import time

import numpy as np
import pytest

from gcn10_amd import gpu
from tests import rainsutil as rs
from tests.test_gpu_aggregate import Inputs, scene  # noqa: F401  (the recipe and the fixture)
from tests.test_gpu_capped_grids import (RAIN_ITEM_COLS, RAIN_ITEM_ROWS, RAIN_NARROW_BANDS, RAIN_TABLES, RAIN_TALL,
                                         OnePairStrip, cus, full_item_landcover, full_item_maps,  # noqa: F401
                                         full_item_preconditions, full_item_tables, full_item_triples,
                                         rain_band_rows, rain_full_item_shape, rain_narrow_shape, rain_tall_celly)
from tests.test_gpu_grid import maps

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("band", RAIN_NARROW_BANDS)
def test_a_narrow_strip_in_tall_bands(scene, tables, cus, band):  # noqa: F811
    """Every row of a tall band must be summed, in cells smaller than a band and in one that several bands add to; then
    ADD semantics and a cut inside a band and inside the tall cell.  One condition, three tables, two layers."""
    assert gpu.grid_rain_item() == (RAIN_ITEM_COLS, RAIN_ITEM_ROWS)
    s = rain_narrow_shape(cus, band)
    print("grid_sums_rains narrow: %s" % s.regime)
    t0 = time.perf_counter()
    inp = Inputs(s.W, s.rows, 25, 29 + band, tables)
    sc = scene(inp)
    t_setup = time.perf_counter() - t0
    cond_mask, table_mask = 1, 0x111
    tall_y, big = rain_tall_celly(s.rows, s.band_rows)
    pairs = [maps(s.W, s.rows, 8, 25.6, (0, 3), (0, 2)), maps(s.W, s.rows, 1e6, 1e6, (0, 3), (0, 2)),
             (maps(s.W, s.rows, 8, 25.6)[0], tall_y)]
    t0 = time.perf_counter()
    for i, (cellx, celly) in enumerate(pairs):
        assert cellx[-1] >= 0 and celly[0] == -1 and celly[-1] == -1
        ncx, ncy = int(cellx.max()) + 1, int(celly.max()) + 1
        fields = rs.fields_for(2, ncx, ncy, 5 + i)
        got = rs.check_rains(sc, cellx, celly, fields, RAIN_TABLES, cond_mask, table_mask)
        assert got.shape == (3, ncy, ncx, 4) and got[..., 1].max() > 0 and (got[..., 2:].max(axis=(0, 1, 2)) > 0).all()
    t_checks = time.perf_counter() - t0
    t0 = time.perf_counter()
    twice = rs.run_rains(sc, cellx, celly, fields, RAIN_TABLES, cond_mask, table_mask, repeat=2)
    np.testing.assert_array_equal(twice, 2 * got)
    y = np.flatnonzero(celly == big)
    cut = int(y[0]) + RAIN_TALL // 2
    cut += cut % s.band_rows == 0
    assert celly[cut - 1] == celly[cut] == big and cut % s.band_rows != 0
    parts = rs.run_rains(sc, cellx, celly, fields, RAIN_TABLES, cond_mask, table_mask,
                         bands=[(0, cut), (cut, s.rows - cut)])
    np.testing.assert_array_equal(parts, got)
    t_runs = time.perf_counter() - t0
    print("grid_sums_rains narrow band=%d: inputs and scene %.2f s, three checks against the oracle %.2f s, two runs of "
          "the device alone (three calls, two downloads) %.2f s; the cut: rows %d + %d in bands of %d and %d" % (
              band, t_setup, t_checks, t_runs, cut, s.rows - cut, rain_band_rows(s.W, cut, cus),
              rain_band_rows(s.W, s.rows - cut, cus)))


def test_full_items_at_the_16_and_32_bit_bounds(scene, cus):  # noqa: F811
    """Items of 512 x 127 pixels: a count of 65 024 in one bin, one of 32 768, and a 32-bit layer sum of 65 024 x
    65 535 in a piece and in the wave's total, in whichever layer names table a.  Then the same strip with rows for the
    clamp: no item may grow to 128 rows."""
    assert gpu.grid_rain_item() == (RAIN_ITEM_COLS, RAIN_ITEM_ROWS)
    s = rain_full_item_shape(cus)
    print("grid_sums_rains full items: %s" % s.regime)
    t0 = time.perf_counter()
    inp = OnePairStrip(full_item_landcover(s.W, s.rows_clamp))
    full_item_preconditions(inp)
    t_host = time.perf_counter() - t0
    t0 = time.perf_counter()
    sc = scene(inp)
    sc.eng.sync()
    t_up = time.perf_counter() - t0
    w = full_item_tables()
    cond_mask, table_mask = 3, 0x11
    t_dev = t_ref = 0.0
    cases = list(full_item_maps(s.W, s.rows).items())
    cases.append(("one cell, table a, rows for the clamp", full_item_maps(s.W, s.rows_clamp)["one cell, table a"]))
    rng = np.random.default_rng(12)
    for name, (cellx, celly, field) in cases:
        # layer 0: the field of the one-raster test; layers 1 and 2: other draws from the three tables
        fields = np.stack([field] + [rng.integers(0, 3, field.shape).astype(np.uint8) for _ in range(2)])
        if name.startswith("one cell"):
            fields[:, 0, 0] = (0, 1, 0)                         # table a in layers 0 and 2
        t0 = time.perf_counter()
        got = rs.run_rains(sc, cellx, celly, fields, w, cond_mask, table_mask)      # the first len(celly) rows
        t1 = time.perf_counter()
        want = np.empty(got.shape, np.int64)
        for j in range(3):
            triples = full_item_triples(inp, cellx, celly, fields[j], w, 4)
            want[..., :2] = triples[..., :2]
            want[..., 2 + j] = triples[..., 2]
        t_dev, t_ref = t_dev + t1 - t0, t_ref + time.perf_counter() - t1
        rs.same_words(got, want, name)
        if name.startswith("one cell"):
            rows = len(celly)
            k = int((inp.rare[:, 0] < rows).sum())
            assert got.shape == (4, 1, 1, 5) and got[0, 0, 0, 1] == s.W * rows
            assert got[0, 0, 0, 2] == got[0, 0, 0, 4] == 65535 * (s.W * rows - k) + k > 2 ** 32
            assert got[0, 0, 0, 3] != got[0, 0, 0, 2]
    print("grid_sums_rains full items: landcover and reference set-up %.2f s, upload and prepare %.2f s, %d runs of the "
          "device (maps up, kernel, words down) %.2f s, closed forms %.2f s" % (t_host, t_up, len(cases), t_dev, t_ref))
