"""GPU: gcn10_gpu_runoff_strip past the first trip of its capped grid, in the manner of tests/test_gpu_capped_grids.py.
The launch is capped at the workgroups resident at once (gcn10_runoff_strip.hip: grid_cap(ctx, per_cu), a multiple of 8)
and every workgroup loops over chunks of 16 px per thread in XCD slabs, so the strips of tests/test_gpu_runoff_strip.py
all end in the first trip.  Here the shape is computed from the device's CU count so that EVERY workgroup makes two trips
and half of them three -- asserted before the launch -- for the 256-thread form (k = 2) and the 1024-thread form (k = 256).
One raster, against numpy over the oracle's raster.  Needs an MI355X."""
import numpy as np
import pytest

from tests import soil_readers as sr
from tests.test_gpu_runoff_strip import Run
from tests.test_gpu_soil_tables import eng9  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

LDS_PER_CU = 160 * 1024         # MI355X
LUT16_BYTES = 6 * (256 * 16 + 16)
W = 4099                        # a lane straddles a row end in most rows


def launch_shape(n_cus, k):
    """(threads, workgroups at most) of gcn10_gpu_runoff_strip with k byte tables"""
    large = k > 32
    lds = LUT16_BYTES + (k + 1) * 260
    per_cu = max(1, min(1 if large else 4, LDS_PER_CU // lds))
    cap = n_cus * per_cu
    cap -= cap % 8
    return (1024 if large else 256), max(cap, 8)


def trips(nchunks, grid):
    """trips of every workgroup by the rule of first_chunk with XCD slabs"""
    if grid % 8 or nchunks < grid:
        return [len(range(b, nchunks, grid)) for b in range(grid)]
    per, step = -(-nchunks // 8), grid // 8
    out = []
    for b in range(grid):
        lo = (b & 7) * per
        hi = min(lo + per, nchunks)
        out.append(len(range(lo + (b >> 3), hi, step)))
    return out


def rows_for(n_cus):
    """rows of a strip W wide whose chunks are 2.5 per workgroup in both forms"""
    threads, grid = launch_shape(n_cus, 2)
    nchunks = 8 * (2 * (grid // 8) + grid // 16)
    return nchunks * threads * 16 // W


@pytest.mark.parametrize("k", [2, 256])
def test_every_workgroup_makes_two_trips_and_some_three(eng9, tables, k):
    n_cus = eng9.device_info()["cus"]
    H = rows_for(n_cus)
    threads, grid = launch_shape(n_cus, k)
    nchunks = -(-(W * H) // (threads * 16))
    t_all = trips(nchunks, grid)
    assert nchunks > grid and min(t_all) == 2 and max(t_all) == 3 and t_all.count(3) >= grid // 4, \
        (n_cus, k, H, nchunks, grid, min(t_all), max(t_all))
    t = sr.ReaderTile(eng9, tables, 4242, W, H, 170, 97, key="runoff-trips-%d" % H)
    rn = None
    try:
        t.prepare()
        rn = Run(t, "37.3", "37.3", k, masks=(2, 1 << 4))
        rn.launch()
        rn.check("k = %d, %d chunks on %d workgroups" % (k, nchunks, grid))
        assert eng9.last_kernel_name() == "runoff_strip_kernel<%d>" % threads
        want = rn.want(13)
        assert len(np.unique(want)) > 20            # the strip means something
    finally:
        eng9.sync()
        if rn is not None:
            rn.close()
        t.close()
