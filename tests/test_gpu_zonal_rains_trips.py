"""GPU: gcn10_gpu_zonal_sums_rains past its first trip.  The grid is capped at 4 workgroups per compute unit; items of 16 px
over every pixel of a strip make n_items >= 2 x cap + 1, so every workgroup takes at least two items, and the test's own
assertion requires that the (zone, tuple) changes inside some workgroups' runs and not inside others.  k = 8.  Expected
values: the oracle's rasters summed in numpy (tests/test_gpu_zonal_rains.py)."""
import numpy as np
import pytest

from gcn10_amd import host
from tests.test_gpu_zonal_rain import scene, strip_inputs  # noqa: F401
from tests.test_gpu_zonal_rains import check

pytestmark = pytest.mark.gpu

PER_CU = 4                  # gcn10_zonal_rain_walk.hpp: grid_cap(ctx, kGridPerCu)
K = 8


def test_more_items_than_twice_the_workgroups(scene, tables, engine):  # noqa: F811
    W = 1040
    cap = PER_CU * int(engine.device_info()["cus"])
    per_row = W // 16
    rows = -(-(2 * cap + 1) // per_row)
    inp = strip_inputs((W, rows, "cap"), W, rows, tables, seed=rows)
    sc = scene(inp)
    src = np.array([(y, 0, W, y % 37) for y in range(rows)], host.ZONE_SPAN_DTYPE)
    src = src[np.lexsort((src["y"], src["zone"]))]
    cellx, celly = (np.arange(W) // 48).astype(np.int32), (np.arange(rows) // 3).astype(np.int32)
    rng = np.random.default_rng(9)
    shape = (int(celly.max()) + 1, int(cellx.max()) + 1)
    # layers of few bytes, so that tuples repeat across the cells of a zone, and a last layer of all bytes
    fields = np.stack([rng.integers(0, 2, shape) * (31 * (j + 1)) for j in range(K - 1)] + [rng.integers(0, 256, shape)])
    fields[-1][rng.integers(0, 2, shape) == 0] = 7
    cut = host.zone_rains_cut({"spans": src}, W, rows, {"cellx": cellx, "celly": celly, "cx0": 0, "cy0": 0},
                              fields.astype(np.uint8), 16, 16)
    items = cut["items"]
    assert len(items) >= 2 * cap + 1
    assert int(cut["rain_pixels"].sum()) == W * rows
    tuples = np.unique(items["table"], axis=0)
    assert len(tuples) > 100 and len(np.unique(tuples[:, :K - 1], axis=0)) < len(tuples)   # some differ in the last layer only
    keys = [(int(z), bytes(t)) for z, t in zip(cut["spans"]["zone"][items["first_span"]], items["table"])]
    per_wg = -(-len(keys) // cap)
    changes = [len(set(keys[a:a + per_wg])) > 1 for a in range(0, len(keys), per_wg)]
    assert per_wg >= 2 and sum(changes) > len(changes) // 4 and not all(changes)       # runs with and without a change
    check(sc, cut["spans"], items, 37, K, cond_mask=1, table_mask=0b11)
