"""GPU: every kernel whose grid is capped by the device's size, run past its first trip.  Needs an MI355X (all tests
but three, which are arithmetic and numpy and run anywhere).

Several kernels launch at most a multiple of the compute-unit count of workgroups; beyond that a workgroup loops over
further work and carries state from trip to trip -- the verifier's tally in LDS and its 64-bit minimum, the pair
histogram's LDS bins --, or strides over a flat array (grid_finish, stream_copy); in gcn10_gpu_grid_sums and in
gcn10_gpu_grid_sums_rain the device's size sets the rows of a band instead.  Every production call on 256 CUs is deep in
that regime; the other kernel tests stay below the caps (one trip per workgroup, bands of the 16-row floor).  This
module computes each shape from the device's CU count with the launch arithmetic of the sources, restated below beside
the constant it mirrors, asserts from that arithmetic that the shape reaches the regime it names, and then compares
exactly: the verifier with numpy on the oracle's rasters (strip form) or on random bytes (buffer form), the histogram
with the numpy model of tests/test_gpu_stats.py, grid_finish with gridutil.means / runoffutil.cn_array and plain
indexing, the weighted grid sums with np.bincount over the oracle's rasters, stream_copy byte for byte.  No tolerance
anywhere.

The rain sums (gcn10_grid_rain.hip, section 6): the launch is not capped, but the band height -- the rows of an item --
is ceil(rows / (16 x CUs // chunks + 1)) held between 16 and 127, and a block's rows in one call (36 000 x 36 000 on 256 CUs)
make every item the full 512 x 127 = 65 024 pixels, on which the kernel's 16-bit counts and 32-bit sums rest.  Bands of
17, 127 and "128" rows (the clamp) run on a strip of 17 columns against the summed oracle of tests/test_gpu_grid_rain.py;
items of 512 x 127 run on a strip of 528 columns whose landcover and soil are made so that one item holds ONE pair
65 024 times and another a bin of 32 768 -- asserted from the arrays --, with a table of 65 535, so that a piece's and
the wave's 32-bit sum is 4 261 347 840, and against a closed form that is itself held to the summed oracle on a cut-out.

Not reached: bands of 256 rows (kMaxBandRows) at block width.  At the 36001 columns of a block they take about 350 Mpx
in one call, and no short test can hold that; the 36001-wide test here reaches bands of 20 rows, the first regime above
the floor of 16, in the weighted launch only (the unweighted launch of the same strip has a third of the roles and
stays at the floor).  Both launches' band arithmetic up to the clamp at 256 rows is run on a strip of 17 columns, where a
band is short -- and where a chunk's 32-bit sums stay far from the bound that 4096 columns x 256 rows come near.
"""
import time
import types

import numpy as np
import pytest

from gcn10_amd import gpu, host
from oracle import cn_oracle_c as oc
from tests import aggutil as au
from tests import gridutil as gu
from tests import rainutil as rn
from tests import runoffutil as ru
from tests import stormutil
from tests.test_gpu_aggregate import Inputs, scene  # noqa: F401  (the recipe and the fixture)
from tests.test_gpu_grid import check_sums, maps, run_finish, run_sums
from tests.test_gpu_grid_rain import TABLES as RAIN_TABLES
from tests.test_gpu_grid_rain import check_rain, field_for, map_of, run_rain, want_rain
from tests.test_gpu_grid_runoff import Q50, WEIGHTS, check_weighted, run_finish_weighted
from tests.test_gpu_stats import landcover, model_histogram
from tests.test_gpu_verify import plant, strips_of
from tests.test_runoff_host import hand_made_triples
from tests.util import HSG_NASTY, make_block

on_gpu = pytest.mark.gpu
NONE = gpu.VERIFY_NONE
POISON, GUARD = 0xA5, 256

# ---- the launch arithmetic of the sources ------------------------------------------------------------------------
THREADS = 256               # kThreads of every kernel here
PX_PER_LANE = 16            # kPxPerLane: pixels of a column group
VERIFY_PER_CU = 4           # gcn10_verify.hip kGridPerCu
HIST_PER_CU = 4             # gcn10_stats.hip kGridPerCu
HIST_CHUNK = 4096           # gcn10_stats.hip kChunk: pixels of a row per workgroup step
HIST_ROWS = 4               # gcn10_stats.hip kRowsPerItem
STREAM_PER_CU = 16          # Opt::grid_blocks_per_cu, the default (gcn10_gpu_internal.hpp)
COPY_TRIP_VECTORS = 512     # stream_copy_kernel: two chunks of kThreads 16-byte vectors per trip
GRID_PER_CU = 8             # launch_sums of gcn10_grid.hip: grid_cap(ctx, 8)
GRID_CHUNK = 4096           # gcn10_grid.hip kChunkPx
BAND_FLOOR, BAND_MAX = 16, 256      # launch_sums: min(max(.., 16), kMaxBandRows)
N_RASTERS = 18
NARROW_BANDS = (17, 257)    # bands asked of the 17-column strips: the first above the floor, and one past kMaxBandRows
RAIN_PER_CU = 16            # gcn10_gpu_grid_sums_rain of gcn10_grid_rain.hip: grid_cap(ctx, 16)
RAIN_ITEM_COLS = 512        # GCN10_GPU_RAIN_ITEM_COLS (kItemCols): columns of an item, and of a chunk of the strip
RAIN_ITEM_ROWS = 127        # GCN10_GPU_RAIN_ITEM_ROWS (kItemRows): the most rows of a band
RAIN_FLOOR = 16             # kMinBandRows
RAIN_NARROW_BANDS = (17, 127, 128)  # of the 17-column strips: the first above the floor, kItemRows, and one past it
RAIN_TALL = 2 * RAIN_ITEM_ROWS + 10     # rows of a cell that at least three bands of any height add to
LC, LC_RARE, CN, CN_RARE = 40, 41, 100, 7   # the full items' two landcover bytes and what their tables make of them


def ceil_div(a, b):
    return -(-a // b)


def grid_cap(cus, per_cu):
    """gcn10_context.hip grid_cap"""
    return cus * per_cu


def stream_grid(cus, nchunks, per_cu=STREAM_PER_CU):
    """gcn10_context.hip stream_grid: the cap is a multiple of 8 (one slab per XCD), 8 at least"""
    cap = cus * per_cu
    cap = max(cap - cap % 8, 8)
    return max(min(nchunks, cap), 1)


def trips_per_workgroup(trips, grid):
    """(fewest, most) trips of a workgroup in `for (trip = blockIdx.x; trip < trips; trip += gridDim.x)`"""
    return trips // grid, ceil_div(trips, grid)


def verify_launch(W, rows, cus):
    """fill_shape and grid_for of gcn10_verify.hip, and the trip loops of the two kernels"""
    s = types.SimpleNamespace(W=W, rows=rows, groups_per_row=W // PX_PER_LANE)
    s.n_groups = rows * s.groups_per_row
    s.trips = ceil_div(s.n_groups, THREADS)
    s.tail = W - s.groups_per_row * PX_PER_LANE
    s.n_tail = s.tail * rows
    s.tail_trips = ceil_div(s.n_tail, THREADS)
    s.cap = grid_cap(cus, VERIFY_PER_CU)
    s.grid = max(min(max(s.trips, s.tail_trips), s.cap), 1)
    return s


def CUTS(H):
    """the block cut into three strips; the middle one keeps the regime"""
    return [1, H - 2]


def verify_shape(name, cus):
    """Shape A: 65 groups and a 15-pixel tail per row, rows for 2 cap + 4 vector trips and a partly dead last one.
    Shape B: one group and a 15-pixel tail per row, rows for a second trip of the tail loop."""
    if name == "A":
        W, cap = 1055, grid_cap(cus, VERIFY_PER_CU)
        rows = ceil_div((2 * cap + 3) * THREADS + 1, W // PX_PER_LANE)
        while rows * (W // PX_PER_LANE) % THREADS == 0:
            rows += 1
        s = verify_launch(W, rows, cus)
        s.hs = (rows // 25 + 2, 42)
        mid = verify_launch(W, rows - 3, cus)
        # every workgroup makes at least 2 trips with its tally, workgroups 0..3 make 3, the last trip is partly dead
        assert s.grid == s.cap and s.trips >= 2 * s.grid + 4 and s.n_groups % THREADS != 0
        assert trips_per_workgroup(s.trips, s.grid) == (2, 3)
        assert mid.grid == mid.cap and mid.trips >= 2 * mid.grid + 1           # and so in the middle strip of CUTS
        assert s.tail == 15 and s.tail_trips < s.grid                          # the tail: one trip (shape B's subject)
        s.regime = "vector part: %d trips over %d workgroups, 2 to 3 each, %d live groups in the last; tail: 1 trip" % (
            s.trips, s.grid, s.n_groups - (s.trips - 1) * THREADS)
    else:
        W, cap = 31, grid_cap(cus, VERIFY_PER_CU)
        rows = ceil_div(cap * THREADS + 16 * THREADS, 15)
        while 15 * rows % THREADS == 0:
            rows += 1
        s = verify_launch(W, rows, cus)
        s.hs = (rows // 25 + 2, 3)
        mid = verify_launch(W, rows - 3, cus)
        # the tail loop: every lane of workgroups 0..15 at least comes round a second time; the vector part: one trip
        assert s.grid == s.cap and s.tail == 15 and s.n_tail >= (s.grid + 16) * THREADS and s.n_tail % THREADS != 0
        assert s.n_tail < 2 * s.grid * THREADS and mid.grid == mid.cap and mid.n_tail >= (mid.grid + 15) * THREADS
        assert 4 < s.trips < s.grid
        s.regime = "tail part: %d items over %d workgroups of 256 lanes, 1 to 2 trips each; vector part: %d trips, 1 each" % (
            s.n_tail, s.grid, s.trips)
    s.name, s.H = name, rows
    return s


def hist_shape(name, cus):
    """pair_histogram_kernel: items = ceil(rows / 4) ceil(W / 4096), grid = min(items, 4 CUs)"""
    W = {"17": 17, "4100": 4100}[name]
    cap = grid_cap(cus, HIST_PER_CU)
    per_row = ceil_div(W, HIST_CHUNK)
    rows = HIST_ROWS * (ceil_div(2 * cap + 3, per_row) - 1) + 1             # the last item has one row
    s = types.SimpleNamespace(W=W, rows=rows, per_row=per_row, items=ceil_div(rows, HIST_ROWS) * per_row, cap=cap)
    s.grid = min(s.items, cap)
    # every workgroup adds at least 2 items to its LDS histogram and at least three workgroups add 3
    assert s.grid == cap and s.items >= 2 * s.grid + 3 and trips_per_workgroup(s.items, s.grid) == (2, 3)
    assert rows % HIST_ROWS == 1
    s.regime = "%d items over %d workgroups, 2 to 3 each" % (s.items, s.grid)
    return s


def finish_shape(cus):
    """grid_finish_kernel: grid = stream_grid(ceil(total / 256)), a stride loop over total = n_sel n_cells elements and
    another over n_sel n_shared packed cells"""
    s = types.SimpleNamespace(n_sel=N_RASTERS)
    cap_elements = stream_grid(cus, 1 << 40) * THREADS
    s.n_cells = ceil_div(2 * cap_elements + THREADS + 1, s.n_sel)
    s.n_shared = cap_elements // s.n_sel + 6
    s.total, s.packed = s.n_sel * s.n_cells, s.n_sel * s.n_shared
    s.grid = stream_grid(cus, ceil_div(s.total, THREADS))
    # every lane finishes at least 2 elements, the 257 first lanes (two workgroups) 3; the packed cells pass the cap once
    assert s.grid * THREADS == cap_elements and s.total >= 2 * cap_elements + THREADS + 1
    assert s.total < 3 * cap_elements and cap_elements < s.packed < 2 * cap_elements
    s.regime = "%d elements over %d lanes, 2 to 3 each; %d packed shared cells, 1 to 2 each" % (
        s.total, cap_elements, s.packed)
    return s


def band_rows(W, rows, roles, cus):
    """launch_sums of gcn10_grid.hip"""
    chunks = ceil_div(W, GRID_CHUNK)
    want = grid_cap(cus, GRID_PER_CU) // (chunks * roles) + 1
    return min(max(ceil_div(rows, want), BAND_FLOOR), BAND_MAX)


def bands_shape(cus):
    """grid_sums_kernel, one table, over a 36001-wide strip, both conditions (6 roles): the fewest rows with bands of 20"""
    s = types.SimpleNamespace(W=36001, roles=6, chunks=ceil_div(36001, GRID_CHUNK))
    want = grid_cap(cus, GRID_PER_CU) // (s.chunks * s.roles) + 1
    s.rows = 19 * want + 1
    s.band_rows = band_rows(s.W, s.rows, s.roles, cus)
    s.bands = ceil_div(s.rows, s.band_rows)
    assert s.chunks == 9 and s.W - 8 * GRID_CHUNK == 3233 and BAND_FLOOR < s.band_rows == 20 < BAND_MAX
    assert band_rows(s.W, s.rows - 1, s.roles, cus) == 19 and s.bands >= 2 and s.rows % s.band_rows != 0
    s.unweighted_band_rows = band_rows(s.W, s.rows, 2, cus)
    s.regime = "W=%d rows=%d: %d bands of %d rows in the weighted kernel (%d in the unweighted cross-check)" % (
        s.W, s.rows, s.bands, s.band_rows, s.unweighted_band_rows)
    return s


def narrow_bands_shape(cus, weighted, band):
    """The sums over a strip of 17 columns (one chunk: a whole group and a group of one pixel), one condition -- one role
    per item, three with weights --: the fewest rows with bands of `band` rows, or, for band = 257, rows for the clamp
    to kMaxBandRows.  A chunk of 17 columns leaves the kernel's 32-bit sums far from their bound (4096 x 256 x 255)."""
    s = types.SimpleNamespace(W=17, roles=3 if weighted else 1)
    want = grid_cap(cus, GRID_PER_CU) // s.roles + 1
    s.rows = (band - 1) * want + 1
    s.rows += s.rows % min(band, BAND_MAX) == 0                 # the last band is a cut one
    s.band_rows = band_rows(s.W, s.rows, s.roles, cus)
    s.bands = ceil_div(s.rows, s.band_rows)
    assert s.band_rows == min(band, BAND_MAX) > BAND_FLOOR and ceil_div(s.rows, want) == band
    assert s.bands >= 2 and s.rows % s.band_rows != 0
    s.regime = "W=17 rows=%d: %d bands of %d rows" % (s.rows, s.bands, s.band_rows)
    return s


def rain_band_rows(W, rows, cus):
    """gcn10_gpu_grid_sums_rain of gcn10_grid_rain.hip: the rows of a band, and so of an item"""
    chunks = ceil_div(W, RAIN_ITEM_COLS)
    want = grid_cap(cus, RAIN_PER_CU) // chunks + 1
    return min(max(ceil_div(rows, want), RAIN_FLOOR), RAIN_ITEM_ROWS)


def rain_narrow_shape(cus, band):
    """The rain sums over a strip of 17 columns (one chunk: a whole group and a group of one pixel): the fewest rows
    with bands of `band` rows, or, for band = 128, rows for the clamp to kItemRows.  An item of 17 columns counts 2159
    pixels at most: the band arithmetic alone, far from the 16-bit and 32-bit bounds (rain_full_item_shape)."""
    s = types.SimpleNamespace(W=17)
    want = grid_cap(cus, RAIN_PER_CU) // ceil_div(s.W, RAIN_ITEM_COLS) + 1
    s.rows = (band - 1) * want + 1
    s.rows += s.rows % min(band, RAIN_ITEM_ROWS) == 0           # the last band is a cut one
    s.band_rows = rain_band_rows(s.W, s.rows, cus)
    s.bands = ceil_div(s.rows, s.band_rows)
    assert s.band_rows == min(band, RAIN_ITEM_ROWS) > RAIN_FLOOR and ceil_div(s.rows, want) == band
    assert s.bands >= 2 and s.rows % s.band_rows != 0
    if band > RAIN_ITEM_ROWS:
        assert ceil_div(s.rows, want) > s.band_rows == RAIN_ITEM_ROWS      # the clamp applies
    s.regime = "W=17 rows=%d: %d bands of %d rows" % (s.rows, s.bands, s.band_rows)
    return s


def rain_full_item_shape(cus):
    """The rain sums over the cheapest strip whose items are 512 columns x 127 rows, the size of every item of a
    block-sized call: two chunks (512 columns and one group of 16), the fewest rows with bands of kItemRows.  rows_clamp:
    the fewest rows at which the arithmetic asks for 128 and the clamp holds it to 127; the bands are the same ones."""
    s = types.SimpleNamespace(W=RAIN_ITEM_COLS + PX_PER_LANE, chunks=2)
    s.want = grid_cap(cus, RAIN_PER_CU) // s.chunks + 1
    s.rows = (RAIN_ITEM_ROWS - 1) * s.want + 1
    s.rows_clamp = RAIN_ITEM_ROWS * s.want + 1
    s.band_rows = rain_band_rows(s.W, s.rows, cus)
    s.bands = ceil_div(s.rows, s.band_rows)
    assert s.W == 528 and ceil_div(s.W, RAIN_ITEM_COLS) == s.chunks and s.band_rows == RAIN_ITEM_ROWS
    assert ceil_div(s.rows, s.want) == RAIN_ITEM_ROWS and rain_band_rows(s.W, s.rows - 1, cus) == RAIN_ITEM_ROWS - 1
    assert ceil_div(s.rows_clamp, s.want) == RAIN_ITEM_ROWS + 1 and rain_band_rows(s.W, s.rows_clamp, cus) == RAIN_ITEM_ROWS
    assert s.bands >= 7                                         # bands 3 and 5 are whole ones
    assert RAIN_ITEM_COLS * s.band_rows == 65024
    s.regime = "W=%d rows=%d (%d px): %d bands of %d rows, the last of %d; and rows=%d for the clamp" % (
        s.W, s.rows, s.W * s.rows, s.bands, s.band_rows, s.rows - (s.bands - 1) * s.band_rows, s.rows_clamp)
    return s


def copy_shape(cus):
    """stream_copy_kernel: trips of 512 vectors, grid = stream_grid(trips), the trips dealt in eight slabs (first_chunk of
    gcn10_device_util.hpp) when the grid is a multiple of 8 and there are trips for every workgroup"""
    s = types.SimpleNamespace()
    s.grid = stream_grid(cus, 1 << 40)
    s.ntrips = 2 * s.grid + 8
    s.nvec = (s.ntrips - 1) * COPY_TRIP_VECTORS + 300               # the last trip: one whole chunk, one cut
    s.nbytes = 16 * s.nvec
    assert stream_grid(cus, s.ntrips) == s.grid and s.grid % 8 == 0 and s.ntrips >= s.grid
    per, step = ceil_div(s.ntrips, 8), s.grid // 8
    n = []
    for b in range(s.grid):
        lo = (b & 7) * per
        n.append(len(range(lo + (b >> 3), min(lo + per, s.ntrips), step)))
    assert sum(n) == s.ntrips and min(n) == 2 and max(n) == 3       # every workgroup 2 trips, the first of a slab 3
    s.regime = "%d trips of 8 KiB over %d workgroups in 8 slabs, 2 to 3 each (%d bytes)" % (s.ntrips, s.grid, s.nbytes)
    return s


def regimes(cus):
    """{test: the regime its shape reaches on a device of `cus` compute units}; every shape function asserts its own"""
    out = {"verify %s" % n: verify_shape(n, cus).regime for n in "AB"}
    out.update({"pair_histogram W=%s" % n: hist_shape(n, cus).regime for n in ("17", "4100")})
    out["grid_finish"] = finish_shape(cus).regime
    out["grid_sums_weighted"] = bands_shape(cus).regime
    for weighted in (False, True):
        for band in NARROW_BANDS:
            out["grid_sums%s W=17 band=%d" % ("_weighted" if weighted else "", band)] = \
                narrow_bands_shape(cus, weighted, band).regime
    out["stream_copy"] = copy_shape(cus).regime
    for band in RAIN_NARROW_BANDS:
        out["grid_sums_rain W=17 band=%d" % band] = rain_narrow_shape(cus, band).regime
    out["grid_sums_rain full items"] = rain_full_item_shape(cus).regime
    return out


@pytest.fixture(scope="module")
def cus(engine):
    n = engine.device_info()["cus"]
    print("regimes at %d CUs: %s" % (n, regimes(n)))
    return n


# ---- 1. the verifier ------------------------------------------------------------------------------------------------

def pixel_of_group(s, trip, lane, k):
    """(y, x) of pixel k of the group that lane `lane` takes in trip `trip` (group gi -> trip gi // 256 -> workgroup
    trip % grid)"""
    gi = trip * THREADS + lane
    assert gi < s.n_groups and k < PX_PER_LANE
    return gi // s.groups_per_row, gi % s.groups_per_row * PX_PER_LANE + k


def pixel_of_tail(s, i):
    """(y, x) of item i of the tail loop (item i -> workgroup i // 256 % grid, again at i + grid * 256)"""
    assert i < s.n_tail
    return i // s.tail, s.W - s.tail + i % s.tail


ROLES = dict(three=6, two=11, last=3, pair=(0, 9), tail=14, tail_late=16, both=8, last_tail=1)


def places_for(s, roles=ROLES):
    """{raster: [(y, x)]} with positions from the trip rule, and {raster: count} of what that must give"""
    g, t = s.grid, 2
    places, counts = {}, {}
    if s.trips > t + 2 * g:
        # one workgroup's tally adds over three trips; without the first pixel, `first` comes from a later trip
        three = [pixel_of_group(s, t, 37, 0), pixel_of_group(s, t + g, 200, 15), pixel_of_group(s, t + 2 * g, 255, 7)]
        places[roles["three"]], places[roles["two"]] = three, three[1:]
    live = s.n_groups - (s.trips - 1) * THREADS
    places[roles["last"]] = [pixel_of_group(s, s.trips - 1, live - 1, 9)]          # the last, partly dead trip
    a, b = roles["pair"]
    places[a] = [pixel_of_group(s, min(t + g, s.trips - 2), 64, 3)]                # two rasters in one 16-pixel group
    places[b] = [pixel_of_group(s, min(t + g, s.trips - 2), 64, 12)]
    i = 3 * THREADS + 65
    if s.n_tail > i + g * THREADS:
        # the same in the tail loop: lane 65 of workgroup 3 twice, and the later one alone
        places[roles["tail"]] = [pixel_of_tail(s, i), pixel_of_tail(s, i + g * THREADS)]
        places[roles["tail_late"]] = [pixel_of_tail(s, i + g * THREADS)]
    else:
        places[roles["tail"]] = [pixel_of_tail(s, i)]
    # workgroup 3 finds one pixel in its vector trip and one in its tail trip
    places[roles["both"]] = [pixel_of_group(s, 3, 129, 5), pixel_of_tail(s, 3 * THREADS + 200)]
    if "last_tail" in roles:
        places[roles["last_tail"]] = [pixel_of_tail(s, s.n_tail - 1)]              # the last, partly dead tail trip
    counts = {r: len(set(p)) for r, p in places.items()}
    return places, counts


def sprinkle(want, seed, n=1000):
    """about n pixels of every raster changed at random places"""
    rng = np.random.default_rng(seed)
    got = want.copy()
    for r in range(N_RASTERS):
        ys, xs = rng.integers(0, want.shape[1], n), rng.integers(0, want.shape[2], n)
        got[r, ys, xs] = want[r, ys, xs] + rng.integers(1, 256, n).astype(np.uint8)      # never the value itself
    return got


def expected(want, got, sel=range(N_RASTERS)):
    """The counters by numpy: the number of differing pixels, the smallest (y << 32) | x among them, want and got
    there."""
    exp = np.zeros(N_RASTERS, gpu.VERIFY_COUNT_DTYPE)
    exp["first"] = NONE
    for r in sel:
        d = got[r] != want[r]
        n = int(d.sum())
        if n:
            y, x = divmod(int(d.argmax()), want.shape[2])           # row major: the smallest y, then the smallest x
            exp[r] = (n, (y << 32) | x, int(want[r, y, x]), int(got[r, y, x]))
    return exp


def padded(rasters, pad, seed):
    """[18][H][W + pad] with noise in the padding"""
    n, H, W = rasters.shape
    out = np.empty((n, H, W + pad), np.uint8)
    out[:, :, :W] = rasters
    out[:, :, W:] = np.random.default_rng(seed).integers(0, 256, size=(n, H, pad), dtype=np.uint8)
    return out


@pytest.fixture(scope="module")
def host_blocks(tables):
    """name -> the host side of a verifier block (landcover, soil, maps, the oracle's 18 rasters), made once"""
    made = {}

    def get(s):
        if s.name not in made:
            hsy, hsx = s.hs
            esa, gt, coarse, sgt = make_block(1000 + s.W, s.H, s.W, hsy, hsx, nasty=True)
            ci, cj = host.build_index_maps(gt, sgt, s.W, s.H, hsx, hsy)
            made[s.name] = types.SimpleNamespace(esa=esa, coarse=coarse, ci=ci, cj=cj, hsx=hsx, hsy=hsy,
                                                 want=oc.process_block_mem(esa, gt, coarse, sgt, tables))
        return made[s.name]

    yield get
    made.clear()


class DeviceBlock:
    """A verifier block on the device, the tile prepared; verify() runs the strip form over it."""

    def __init__(self, eng, tables, s, hb):
        self.eng, self.s = eng, s
        eng.set_tables(tables)
        self.bufs = [eng.upload(a) for a in (hb.esa, hb.coarse, hb.ci, hb.cj)]
        eng.prepare_tile(self.bufs[1].ptr, hb.hsx, hb.hsy, self.bufs[2].ptr, s.W)

    def close(self):
        for b in self.bufs:
            b.close()

    def verify(self, got, strips, cond_mask=3, table_mask=0x1FF, pad=23, preset=None):
        """The counters after verify_strip over `strips` of the "file" rasters got (rows W + pad bytes apart); asserts
        that the rasters were not written."""
        eng, H, W = self.eng, self.s.H, self.s.W
        stride = W + pad
        host_got = padded(got, pad, 5)
        dev = eng.upload(host_got)
        counts = eng.verify_counts_alloc()
        try:
            if preset is not None:
                eng.h2d(counts.ptr, preset)
                eng.sync()
            for y0, rows in strips:
                ptrs = [dev.ptr + (r * H + y0) * stride for r in range(N_RASTERS)]
                eng.verify_strip(self.bufs[0].ptr + y0 * W, W, rows, self.bufs[3].ptr + 4 * y0, cond_mask, table_mask,
                                 ptrs, stride, y0, counts.ptr)
            out = eng.verify_counts(counts.ptr)
            after = eng.download(dev.ptr, host_got.shape)
        finally:
            eng.sync()
            dev.close()
            counts.close()
        assert np.array_equal(after, host_got), "the verifier wrote to the file rasters"
        return out


def same_counters(out, exp, what):
    for r in range(N_RASTERS):
        assert out[r].tolist() == exp[r].tolist(), "%s: raster %d: got %s, want %s" % (what, r, out[r], exp[r])


@on_gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_verify_strip_adds_up_over_the_trips(engine, tables, cus, host_blocks, name):
    s = verify_shape(name, cus)
    hb = host_blocks(s)
    blk = DeviceBlock(engine, tables, s, hb)
    try:
        whole, cut = [(0, s.H)], strips_of(s.H, CUTS(s.H))
        assert len(cut) == 3
        out = blk.verify(hb.want, whole)
        assert out["mismatches"].tolist() == [0] * 18 and out["first"].tolist() == [NONE] * 18
        places, counts = places_for(s)
        got, _ = plant(hb.want, places)
        exp = expected(hb.want, got)
        assert {r: int(exp[r]["mismatches"]) for r in places} == counts and int(exp["mismatches"].sum()) == sum(counts.values())
        for strips in (whole, cut):
            out = blk.verify(got, strips)
            print("verify_strip %s planted, %d strips: %s" % (name, len(strips), out["mismatches"].tolist()))
            same_counters(out, exp, "planted, %d strips" % len(strips))
    finally:
        blk.close()


@on_gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_verify_strip_counts_a_sprinkle_over_all_rasters(engine, tables, cus, host_blocks, name):
    s = verify_shape(name, cus)
    hb = host_blocks(s)
    blk = DeviceBlock(engine, tables, s, hb)
    try:
        got = sprinkle(hb.want, 7 + s.W)
        exp = expected(hb.want, got)
        assert (exp["mismatches"] > 900).all()
        for strips in ([(0, s.H)], strips_of(s.H, CUTS(s.H))):
            same_counters(blk.verify(got, strips, pad=0), exp, "sprinkle, %d strips" % len(strips))
    finally:
        blk.close()


@on_gpu
def test_verify_strip_of_a_subset_adds_up_over_the_trips(engine, tables, cus, host_blocks):
    """verify_strip_kernel<false>: eight of the 18 rasters, the others hold garbage and their counters markers"""
    s = verify_shape("A", cus)
    hb = host_blocks(s)
    cond_mask, table_mask = 3, 0x0B1
    sel = [r for r in range(18) if (cond_mask >> (r // 9)) & 1 and (table_mask >> (r % 9)) & 1]
    roles = dict(three=4, two=13, last=5, pair=(0, 9), tail=14, tail_late=16, both=7)
    assert sel == [0, 4, 5, 7, 9, 13, 14, 16]
    places, counts = places_for(s, roles)
    assert set(places) <= set(sel)
    blk = DeviceBlock(engine, tables, s, hb)
    try:
        got, _ = plant(hb.want, places)
        preset = np.zeros(18, gpu.VERIFY_COUNT_DTYPE)
        preset["first"] = NONE
        for r in range(18):
            if r not in sel:
                got[r] = 255 - hb.want[r]
                preset[r] = (1000 + r, 77 + r, 3, 4)
        exp = expected(hb.want, got, sel)
        assert {r: int(exp[r]["mismatches"]) for r in places} == counts
        for r in range(18):
            if r not in sel:
                exp[r] = preset[r]
        same_counters(blk.verify(got, [(0, s.H)], cond_mask, table_mask, preset=preset), exp, "subset")
    finally:
        blk.close()


def run_buffers(eng, d_want, ws, got, W, H, strips, mask=0x3FFFF, pad=32):
    """The counters after verify_buffers over `strips`; asserts that got was not written (want: by the caller, once)."""
    gs = W + pad
    host_got = padded(got, pad, 9)
    dg = eng.upload(host_got)
    counts = eng.verify_counts_alloc()
    try:
        for y0, rows in strips:
            eng.verify_buffers([d_want.ptr + (r * H + y0) * ws for r in range(18)], ws,
                               [dg.ptr + (r * H + y0) * gs for r in range(18)], gs, W, rows, y0, mask, counts.ptr)
        out = eng.verify_counts(counts.ptr)
        assert np.array_equal(eng.download(dg.ptr, host_got.shape), host_got), "verify_buffers wrote to got"
    finally:
        eng.sync()
        dg.close()
        counts.close()
    return out


@on_gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_verify_buffers_adds_up_over_the_trips(engine, cus, name):
    s = verify_shape(name, cus)
    want = np.random.default_rng(s.W).integers(0, 256, size=(18, s.H, s.W), dtype=np.uint8)
    ws = s.W + 7
    host_want = padded(want, 7, 3)
    d_want = engine.upload(host_want)
    try:
        whole, cut = [(0, s.H)], strips_of(s.H, CUTS(s.H))
        out = run_buffers(engine, d_want, ws, want, s.W, s.H, whole)
        assert out["mismatches"].tolist() == [0] * 18 and out["first"].tolist() == [NONE] * 18
        places, counts = places_for(s)
        planted, _ = plant(want, places)
        for what, got in (("planted", planted), ("sprinkle", sprinkle(want, 11 + s.W))):
            exp = expected(want, got)
            if what == "planted":
                assert {r: int(exp[r]["mismatches"]) for r in places} == counts
            for strips in (whole, cut):
                out = run_buffers(engine, d_want, ws, got, s.W, s.H, strips)
                print("verify_buffers %s %s, %d strips: %s" % (name, what, len(strips), out["mismatches"].tolist()))
                same_counters(out, exp, "%s, %d strips" % (what, len(strips)))
        assert np.array_equal(engine.download(d_want.ptr, host_want.shape), host_want), "verify_buffers wrote to want"
    finally:
        engine.sync()
        d_want.close()


# ---- 2. pair_histogram --------------------------------------------------------------------------------------------

@on_gpu
@pytest.mark.parametrize("name", ["17", "4100"])
@pytest.mark.parametrize("pattern", ["one pair", "patchy", "iid"])
def test_pair_histogram_adds_up_over_the_items(engine, cus, name, pattern):
    s = hist_shape(name, cus)
    W, rows = s.W, s.rows
    rng = np.random.default_rng(W + rows)
    esa = landcover(pattern, rows, W, rng)
    hsx, hsy = max(1, W // 25 + 2), max(1, rows // 25 + 2)
    coarse = rng.choice(HSG_NASTY, size=(hsy, hsx)).astype(np.uint8)
    if pattern == "one pair":
        coarse[:] = 3           # one bin for every wave: the wave-wide shortcut of count16, trip after trip
    gt = [0.0, 1.0 / W, 0.0, 1.0, 0.0, -1.0 / W]
    sgt = [-0.013, 1.0 / (hsx - 1.5), 0.0, 1.02, 0.0, -1.0 / (hsy - 1.5)]
    ci, cj = host.build_index_maps(gt, sgt, W, rows, hsx, hsy)
    want = model_histogram(esa, coarse[cj[:, None], ci[None, :]])
    bufs = [engine.upload(a) for a in (esa, coarse, ci, cj)]
    hist = engine.alloc(16 * 256 * 8)
    try:
        engine.prepare_tile(bufs[1].ptr, hsx, hsy, bufs[2].ptr, W)
        engine.memset(hist.ptr, 0, 16 * 256 * 8)
        engine.pair_histogram(bufs[0].ptr, W, rows, bufs[3].ptr, hist.ptr)
        one = engine.download(hist.ptr, (16 * 256,), np.uint64)
        engine.pair_histogram(bufs[0].ptr, W, rows, bufs[3].ptr, hist.ptr)
        two = engine.download(hist.ptr, (16 * 256,), np.uint64)
    finally:
        engine.sync()
        for b in bufs + [hist]:
            b.close()
    np.testing.assert_array_equal(one, want)
    np.testing.assert_array_equal(two, 2 * want)
    assert int(one.sum()) == W * rows
    if pattern == "one pair":
        assert np.count_nonzero(want) == 1


# ---- 3. grid_finish and grid_finish_weighted ------------------------------------------------------------------------

def triple_pool(q, seed=3):
    """int64[n][3] triples {s, n, sw}: the hand-made ones of the host tests (n = 0, sw = 0, exact halves, n = 2^40) and
    random ones of every size of n -- sums beyond 2^32 among them -- with sw at, beside and between the n q[c]."""
    rng = np.random.default_rng(seed)
    m = 4000
    n = np.concatenate([np.zeros(m // 8, np.int64), rng.integers(1, 65, m // 4), rng.integers(1, 1 << 20, m // 4),
                        rng.integers(1 << 31, 1 << 40, m - m // 8 - 2 * (m // 4))])
    rng.shuffle(n)
    v = rng.integers(0, 254, m)
    s = n * v + (rng.random(m) * n).astype(np.int64)
    half = (n > 0) & (n % 2 == 0) & (rng.random(m) < 0.25)
    s = np.where(half, n * v + n // 2, s)                                       # (2 s + n) / (2 n) is a whole number
    qq = np.asarray(q, np.int64)
    at = n * qq[rng.integers(1, 101, m)]
    kind = rng.integers(0, 5, m)
    sw = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [0, at, at + 1, np.maximum(at - 1, 0)],
                   (rng.random(m) * n * int(qq[100])).astype(np.int64))
    sw = np.where(n == 0, rng.integers(0, 9, m), sw)                            # n = 0 wins over any sw
    pool = np.concatenate([np.array(hand_made_triples(q), np.int64), np.stack([s, n, sw], axis=1)])
    assert (pool[:, 0] > (1 << 32)).any() and (pool[:, 2] > (1 << 32)).any() and (pool[:, 1] == 0).any()
    assert ((pool[:, 1] > 0) & (pool[:, 2] == 0)).any() and half.any()
    return pool


@pytest.fixture(scope="module")
def finish_case(cus):
    """(shape, pool, which pool entry every element holds, the shared cells): made once for both finish tests"""
    s = finish_shape(cus)
    rng = np.random.default_rng(17)
    pool = triple_pool(Q50)
    pick = rng.integers(0, len(pool), size=(s.n_sel, s.n_cells))
    k = min(len(pool), s.n_cells)
    pick[:, :k] = np.arange(k)                                  # every pool entry at least once per raster
    idx = rng.integers(0, s.n_cells, s.n_shared).astype(np.uint32)
    idx[:4] = (s.n_cells - 1, 0, 7, 7)                          # the last cell, the first, a repeat
    idx[-1] = s.n_cells - 1
    assert len(np.unique(idx)) < len(idx)
    return s, pool, pick, idx


@on_gpu
def test_grid_finish_strides_over_the_cells(engine, finish_case):
    s, pool, pick, idx = finish_case
    engine.set_option("defaults", 0)                            # grid_blocks_per_cu = 16
    acc = pool[pick][..., :2]
    means, shared = run_finish(engine, acc, idx)
    np.testing.assert_array_equal(means, gu.means(pool[:, :2])[pick])
    np.testing.assert_array_equal(shared, acc[:, idx, :])
    assert (means[acc[..., 1] == 0] == 255).all()


@on_gpu
@pytest.mark.parametrize("table", ["50 mm", "goes down"])
def test_grid_finish_weighted_strides_over_the_cells(engine, tables, finish_case, table):
    s, pool, pick, idx = finish_case
    engine.set_option("defaults", 0)
    engine.set_tables(tables)
    w = Q50.copy()
    if table == "goes down":
        w[40:60] = w[40:60][::-1]                               # not rising: the scan branch of runoff_cn
        assert (np.diff(w[1:101].astype(np.int64)) < 0).any()
    else:
        assert (np.diff(w[1:101].astype(np.int64)) >= 0).all()  # rising: the bisection
    acc = pool[pick]
    means, cnq, shared = run_finish_weighted(engine, acc, idx, w)
    want = ru.cn_array(pool, w)
    assert len(set(want.tolist())) > 50
    np.testing.assert_array_equal(means, gu.means(pool[:, :2])[pick])
    np.testing.assert_array_equal(cnq, want[pick])
    np.testing.assert_array_equal(shared, acc[:, idx, :])


# ---- 4. grid_sums_weighted with bands above the 16-row floor --------------------------------------------------------

@on_gpu
def test_grid_sums_weighted_in_bands_of_twenty_rows(scene, tables, cus):
    s = bands_shape(cus)
    inp = Inputs(s.W, s.rows, 25, 19, tables)
    sc = scene(inp)
    table_mask = 1 << 4                                         # one table, both conditions: six roles per item
    # the usual lead and trail of -1 twice; then none, so that the last group's one pixel is in a cell
    for (wx, wy), lead, trail in (((25.6, 25.6), (5, 3), (3, 2)), ((1e6, 1e6), (5, 3), (3, 2)), ((17.3, 25), (0, 0), (0, 0))):
        cellx, celly = maps(s.W, s.rows, wx, wy, lead, trail)
        assert (cellx[-1] == -1) == (trail[0] > 0) and cellx[8 * GRID_CHUNK] >= 0       # the ninth chunk holds cells
        got = check_weighted(sc, cellx, celly, WEIGHTS["random"], 3, table_mask)
        assert got.shape[0] == 2 and got[..., 1].max() > 0 and got[..., 2].max() > 0
        # words 0 and 1 against the unweighted call on the same maps: a cross-check, not the parity claim
        np.testing.assert_array_equal(got[..., :2], run_sums(sc, cellx, celly, 3, table_mask))
        if wx == 1e6:
            assert got.shape == (2, 1, 1, 3) and got[0, 0, 0, 2] > (1 << 32)


@on_gpu
@pytest.mark.parametrize("band", NARROW_BANDS)
@pytest.mark.parametrize("weighted", [False, True], ids=["sums", "weighted"])
def test_grid_sums_of_a_narrow_strip_in_tall_bands(scene, tables, cus, weighted, band):
    """Both kernels' band arithmetic above the floor and at the clamp to 256 rows, on a strip narrow enough to be short."""
    s = narrow_bands_shape(cus, weighted, band)
    inp = Inputs(s.W, s.rows, 25, 23 + band, tables)
    sc = scene(inp)
    for wx, wy in ((8, 25.6), (1e6, 1e6)):
        cellx, celly = maps(s.W, s.rows, wx, wy, (0, 3), (0, 2))
        assert cellx[-1] >= 0 and (wy == 1e6) == (celly.max() == 0)
        if weighted:
            got = check_weighted(sc, cellx, celly, WEIGHTS["random"], 2, 0x111)
            np.testing.assert_array_equal(got[..., :2], run_sums(sc, cellx, celly, 2, 0x111))
        else:
            got = check_sums(sc, cellx, celly, 1, 0x111)
        assert got.shape[0] == 3 and got[..., 1].max() > 0


# ---- 5. stream_copy -----------------------------------------------------------------------------------------------

@on_gpu
def test_stream_copy_past_the_cap(engine, cus):
    """The only copy of more than CUs x 16 trips in the suite is the 256 MiB delay of tests/test_gpu_soil_readers.py,
    whose bytes nobody reads; this one is compared."""
    s = copy_shape(cus)
    engine.set_option("defaults", 0)
    src = np.random.default_rng(5).integers(0, 256, size=s.nbytes, dtype=np.uint8)
    a, b = engine.upload(src), engine.alloc(s.nbytes + 2 * GUARD)
    try:
        engine.memset(b.ptr, POISON, s.nbytes + 2 * GUARD)
        engine.stream_copy(a.ptr, b.ptr + GUARD, s.nbytes)
        engine.sync()
        got = engine.download(b.ptr, (s.nbytes + 2 * GUARD,))
        assert np.array_equal(engine.download(a.ptr, (s.nbytes,)), src)
    finally:
        engine.sync()
        a.close()
        b.close()
    assert (got[:GUARD] == POISON).all() and (got[-GUARD:] == POISON).all(), "bytes around the copy were written"
    assert np.array_equal(got[GUARD:-GUARD], src)


# ---- 6. grid_sums_rain in items taller than the 16-row floor, up to the full 512 x 127 --------------------------------

def rain_tall_celly(rows, band_rows):
    """(celly, the tall cell nearest the middle): cells of 25 and 26 rows in turn with three rows of -1 behind each, and
    after every forty of them one of RAIN_TALL rows, round and round; -1 for the first 3 rows and the last 2."""
    m = map_of(rows, [25, 3, 26, 3] * 20 + [RAIN_TALL, 3], 3, 2)
    celly = np.where((m >= 0) & (m % 2 == 0), m // 2, -1).astype(np.int32)     # every second run is a gap
    sizes = np.bincount(celly[celly >= 0])
    tall = np.flatnonzero(sizes == RAIN_TALL)
    assert len(tall) >= 3 and set(sizes[:-1].tolist()) == {25, 26, RAIN_TALL} and (celly[3:-2] == -1).any()
    big = int(tall[len(tall) // 2])
    y = np.flatnonzero(celly == big)
    assert len(y) == RAIN_TALL and y[-1] - y[0] == RAIN_TALL - 1
    assert y[-1] // band_rows - y[0] // band_rows >= 2, "the tall cell does not span three bands"
    return celly, big


@on_gpu
@pytest.mark.parametrize("band", RAIN_NARROW_BANDS)
def test_grid_sums_rain_of_a_narrow_strip_in_tall_bands(scene, tables, cus, band):
    """The band arithmetic of the rain sums above the floor, at kItemRows and at the clamp to it, on a strip narrow
    enough to be short: every row of a tall band must be summed, in cells smaller than a band and in one that several
    bands add to.  One condition, three tables: three rasters of the oracle per strip."""
    assert gpu.grid_rain_item() == (RAIN_ITEM_COLS, RAIN_ITEM_ROWS)
    s = rain_narrow_shape(cus, band)
    print("grid_sums_rain narrow: %s" % s.regime)
    t0 = time.perf_counter()
    inp = Inputs(s.W, s.rows, 25, 29 + band, tables)
    sc = scene(inp)
    t_setup = time.perf_counter() - t0
    cond_mask, table_mask = 1, 0x111
    tall_y, big = rain_tall_celly(s.rows, s.band_rows)
    pairs = [maps(s.W, s.rows, 8, 25.6, (0, 3), (0, 2)), maps(s.W, s.rows, 1e6, 1e6, (0, 3), (0, 2)),
             (maps(s.W, s.rows, 8, 25.6)[0], tall_y)]
    t0 = time.perf_counter()
    for k, (cellx, celly) in enumerate(pairs):
        assert cellx[-1] >= 0 and celly[0] == -1 and celly[-1] == -1
        ncx, ncy = int(cellx.max()) + 1, int(celly.max()) + 1
        assert ncx == (1 if k == 1 else 3) and (ncy == 1) == (k == 1)
        field = field_for(ncx, ncy, 5 + k)
        got = check_rain(sc, cellx, celly, field, RAIN_TABLES, cond_mask, table_mask)
        assert got.shape == (3, ncy, ncx, 3) and got[..., 1].max() > 0 and got[..., 2].max() > 0
    t_checks = time.perf_counter() - t0
    # on the last maps: ADD semantics, and a cut inside a band and inside the tall cell
    t0 = time.perf_counter()
    twice = run_rain(sc, cellx, celly, field, RAIN_TABLES, cond_mask, table_mask, repeat=2)
    np.testing.assert_array_equal(twice, 2 * got)
    y = np.flatnonzero(celly == big)
    cut = int(y[0]) + RAIN_TALL // 2
    cut += cut % s.band_rows == 0
    assert celly[cut - 1] == celly[cut] == big and cut % s.band_rows != 0
    parts = run_rain(sc, cellx, celly, field, RAIN_TABLES, cond_mask, table_mask, bands=[(0, cut), (cut, s.rows - cut)])
    np.testing.assert_array_equal(parts, got)
    t_runs = time.perf_counter() - t0
    print("grid_sums_rain narrow band=%d: inputs and scene %.2f s, three checks against the oracle %.2f s, two runs of "
          "the device alone (three calls, two downloads) %.2f s; the cut: rows %d + %d in bands of %d and %d" % (
              band, t_setup, t_checks, t_runs, cut, s.rows - cut, rain_band_rows(s.W, cut, cus),
              rain_band_rows(s.W, s.rows - cut, cus)))


class OnePairStrip:
    """What Scene reads of a strip -- and want_rain, on a small one -- for a landcover array over ONE valid soil class
    and tables with two values: CN everywhere, CN_RARE for landcover LC_RARE."""

    def __init__(self, esa):
        self.esa = np.ascontiguousarray(esa)
        self.rows, self.W = self.esa.shape
        self.tables = np.full((9, 256, 5), CN, np.int32)
        self.tables[:, LC_RARE, :] = CN_RARE
        self.hsx, self.hsy = int(self.W / 25) + 2, int(self.rows / 25) + 3
        self.coarse = np.full((self.hsy, self.hsx), 2, np.uint8)            # a valid soil everywhere: no pixel is 255
        gt = [0.0, 1.0 / self.W, 0.0, 1.0, 0.0, -1.0 / self.W]
        sgt = [-0.013 * 25 / self.W, 25 / self.W, 0.0, 1.0 + 0.02 * 25 / self.W, 0.0, -25 / self.W]
        self.ci, self.cj = host.build_index_maps(gt, sgt, self.W, self.rows, self.hsx, self.hsy)
        self.rare = np.argwhere(self.esa == LC_RARE)                        # (y, x) of every LC_RARE pixel
        self._want = {}

    def want(self, r):
        if r not in self._want:
            self._want.update(au.oracle_rasters(self.esa, np.full(self.esa.shape, 2, np.uint8), self.tables, [r]))
        return self._want[r]


def full_item_landcover(W, rows, seed=41, n_rare=4000):
    """uint8[rows][W]: LC everywhere, but (a) LC_RARE at n_rare random places, none in bands 3 and 5 of chunk 0, and
    (b) LC_RARE in the upper 64 rows of band 5 of chunk 0 -- bands of RAIN_ITEM_ROWS rows, chunks of RAIN_ITEM_COLS."""
    rng = np.random.default_rng(seed)
    esa = np.full((rows, W), LC, np.uint8)
    ys, xs = rng.integers(0, rows, n_rare), rng.integers(0, W, n_rare)
    keep = ~(np.isin(ys // RAIN_ITEM_ROWS, (3, 5)) & (xs < RAIN_ITEM_COLS))
    esa[ys[keep], xs[keep]] = LC_RARE
    esa[5 * RAIN_ITEM_ROWS:5 * RAIN_ITEM_ROWS + 64, :RAIN_ITEM_COLS] = LC_RARE
    return esa


def full_item_preconditions(inp):
    """The point of the full-item test, asserted from the arrays: the item of band 3 / chunk 0 holds one single pair
    over all its 65 024 pixels, the one of band 5 exactly two bins, of 32 768 (bit 15 alone) and 32 256."""
    assert (inp.coarse == 2).all()
    item = inp.esa[3 * RAIN_ITEM_ROWS:4 * RAIN_ITEM_ROWS, :RAIN_ITEM_COLS]
    assert item.shape == (RAIN_ITEM_ROWS, RAIN_ITEM_COLS) and item.size == 65024 and (item == LC).all()
    item = inp.esa[5 * RAIN_ITEM_ROWS:6 * RAIN_ITEM_ROWS, :RAIN_ITEM_COLS]
    bins = np.bincount(item.reshape(-1), minlength=256)
    assert item.shape == (RAIN_ITEM_ROWS, RAIN_ITEM_COLS) and np.count_nonzero(bins) == 2
    assert (bins[LC_RARE], bins[LC]) == (32768, 32256) and 32768 == 1 << 15
    assert len(inp.rare) > 32768 + 2000                             # and the sprinkle of (a) is there


def full_item_tables():
    """uint16[3][256]: `a` (65535 for the common value, 1 for the rare one, else 0), the 50 mm table, a random one"""
    a = np.zeros(256, np.uint16)
    a[CN], a[CN_RARE] = 65535, 1
    return np.stack([a, Q50, stormutil.POOL["random"]])


def full_item_triples(inp, cellx, celly, field, w, n_sel):
    """int64[n_sel][ncy][ncx][3] in closed form, no pixel visited but the LC_RARE ones: with n pixels in a cell and k of
    them LC_RARE, s = CN (n - k) + CN_RARE k and sw = w[CN] (n - k) + w[CN_RARE] k for the table w the cell's byte names."""
    ncy, ncx = field.shape
    assert celly.max() == ncy - 1 and cellx.max() == ncx - 1 and len(cellx) == inp.W
    n = np.outer(np.bincount(celly[celly >= 0], minlength=ncy), np.bincount(cellx[cellx >= 0], minlength=ncx)).astype(np.int64)
    at = inp.rare[inp.rare[:, 0] < len(celly)]
    cy, cx = celly[at[:, 0]], cellx[at[:, 1]]
    k = np.zeros((ncy, ncx), np.int64)
    np.add.at(k, (cy[(cy >= 0) & (cx >= 0)], cx[(cy >= 0) & (cx >= 0)]), 1)
    wt = np.asarray(w, np.int64)[rn.clamp_field(field, len(w))]     # [ncy][ncx][256]
    acc = np.stack([CN * (n - k) + CN_RARE * k, n, wt[..., CN] * (n - k) + wt[..., CN_RARE] * k], axis=-1)
    return np.broadcast_to(acc, (n_sel,) + acc.shape)


def rain_edge_cellx(W):
    """cell edges at 16 k + 7 (inside a lane's 16 pixels) and at 512 (between two items), -1 columns around"""
    assert W == RAIN_ITEM_COLS + PX_PER_LANE
    m = np.full(W, -1, np.int32)
    for k, (a, b) in enumerate(((7, 23), (23, 231), (231, RAIN_ITEM_COLS), (RAIN_ITEM_COLS, 519), (521, W - 2))):
        m[a:b] = k
    return m


def full_item_maps(W, rows, seed=6):
    """{name: (cellx, celly, field)}, the field's bytes naming the three tables of full_item_tables"""
    rng = np.random.default_rng(seed)
    out = {"one cell, table a": (np.zeros(W, np.int32), np.zeros(rows, np.int32), None),
           "120 x 50": maps(W, rows, 120, 50, (5, 3), (3, 2)) + [None],
           "8 columns, the whole height": maps(W, rows, 8, 1e6) + [None],
           "edges at 16 k + 7 and at 512": (rain_edge_cellx(W), map_of(rows, (300,), 3, 2), None)}
    for name, (cellx, celly, _) in out.items():
        shape = (int(celly.max()) + 1, int(cellx.max()) + 1)
        field = np.zeros(shape, np.uint8) if name.startswith("one cell") else rng.integers(0, 3, shape).astype(np.uint8)
        assert field.size < 30 or len(np.unique(field)) == 3
        out[name] = (cellx, celly, field)
    return out


def same_triples(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d of %d words differ, first (q, cy, cx, word) = %s: got %d, want %d" % (
        what, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def test_the_closed_form_of_the_full_items_is_the_summed_oracle(tables):
    """No GPU: full_item_triples against want_rain (the oracle's rasters, summed) on 528 x 300 pixels cut out of the
    recipe where it holds both landcover bytes, and what the pure item alone gives to one cell with table a."""
    whole = OnePairStrip(full_item_landcover(528, 7 * RAIN_ITEM_ROWS + 11))
    full_item_preconditions(whole)
    y0 = 3 * RAIN_ITEM_ROWS + 100                       # the end of band 3, band 4, and (b) of band 5 with rows below
    inp = OnePairStrip(whole.esa[y0:y0 + 300])
    n_rare = len(inp.rare)
    assert (inp.W, inp.rows) == (528, 300) and 64 * 512 + 100 < n_rare < 64 * 512 + 3000 and (inp.esa == LC).sum() == 528 * 300 - n_rare
    w = full_item_tables()
    assert w[0][CN] == 65535 and w[0][CN_RARE] == 1 and w[0].sum() == 65536 and len({t.tobytes() for t in w}) == 3
    for name, (cellx, celly, field) in full_item_maps(528, 300).items():
        want = want_rain(inp, cellx, celly, field, w, 3, 0x11)
        assert want.shape[0] == 4 and want[..., 2].max() > 0
        same_triples(full_item_triples(inp, cellx, celly, field, w, 4), want, name)
    # one condition's values are the other's and a table's another's: CN and CN_RARE, nothing else
    assert all(set(np.unique(inp.want(r)).tolist()) == {CN, CN_RARE} for r in (0, 4, 9, 13))
    item = OnePairStrip(whole.esa[3 * RAIN_ITEM_ROWS:4 * RAIN_ITEM_ROWS, :RAIN_ITEM_COLS])
    one = full_item_triples(item, np.zeros(512, np.int32), np.zeros(RAIN_ITEM_ROWS, np.int32), np.zeros((1, 1), np.uint8), w, 1)
    assert one[0, 0, 0].tolist() == [6502400, 65024, 4261347840] and 4261347840 == 65024 * 65535 < 2 ** 32
    assert 2 ** 32 - 4261347840 < 2 ** 32 // 100        # within 1 % of the bound


@on_gpu
def test_grid_sums_rain_of_full_items_at_the_16_and_32_bit_bounds(scene, cus):
    """Items of 512 x 127 pixels, what every item of a block-sized call is: a count of 65 024 in one bin, one of 32 768,
    and a 32-bit sum of 65 024 x 65 535 -- 0.8 % below 2^32 -- in a piece and in the wave's total.  Then the same
    strip with rows for the clamp: no item may grow to 128 rows, which would carry a count into the bin field."""
    assert gpu.grid_rain_item() == (RAIN_ITEM_COLS, RAIN_ITEM_ROWS)
    s = rain_full_item_shape(cus)
    print("grid_sums_rain full items: %s" % s.regime)
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
    for name, (cellx, celly, field) in cases:
        t0 = time.perf_counter()
        got = run_rain(sc, cellx, celly, field, w, cond_mask, table_mask)       # the first len(celly) rows
        t1 = time.perf_counter()
        want = full_item_triples(inp, cellx, celly, field, w, 4)
        t_dev, t_ref = t_dev + t1 - t0, t_ref + time.perf_counter() - t1
        same_triples(got, want, name)
        if name.startswith("one cell"):
            rows = len(celly)
            k = int((inp.rare[:, 0] < rows).sum())
            assert got.shape == (4, 1, 1, 3) and got[0, 0, 0, 1] == s.W * rows
            assert got[0, 0, 0, 2] == 65535 * (s.W * rows - k) + k > 2 ** 32
    print("grid_sums_rain full items: landcover and reference set-up %.2f s, upload and prepare %.2f s, %d runs of the "
          "device (maps up, kernel, triples down) %.2f s, closed forms %.2f s" % (t_host, t_up, len(cases), t_dev, t_ref))


# ---- the fast path of the expected sums (no GPU) ----------------------------------------------------------------

def test_the_bincount_path_adds_what_add_at_adds(monkeypatch):
    """gridutil.add_words_bincount, which add_sums and add_triples take from two million pixels on, against their
    np.add.at form on a raster small enough for both"""
    rng = np.random.default_rng(2)
    W, rows = 333, 77
    raster = rng.choice(np.array([0, 1, 77, 100, 254, 255], np.uint8), size=(rows, W))
    cellx, celly = maps(W, rows, 8.5, 17.3, (2, 1), (1, 2))
    w = WEIGHTS["random"]
    slow = np.zeros((int(celly.max()) + 1, int(cellx.max()) + 1, 3), np.int64)
    ru.add_triples(slow, raster, cellx, celly, w)
    assert raster.size < gu.BINCOUNT_FROM and slow[..., 1].max() > 0 and (raster == 255).any()
    monkeypatch.setattr(gu, "BINCOUNT_FROM", 0)
    fast, pairs = np.zeros_like(slow), np.zeros_like(slow[..., :2])
    ru.add_triples(fast, raster, cellx, celly, w)
    gu.add_sums(pairs, raster, cellx, celly)
    np.testing.assert_array_equal(fast, slow)
    np.testing.assert_array_equal(pairs, slow[..., :2])
    ru.add_triples(fast, raster, cellx, celly, w)               # it ADDS
    np.testing.assert_array_equal(fast, 2 * slow)


# ---- the regimes, from the arithmetic alone (no GPU) --------------------------------------------------------------

@pytest.mark.parametrize("n_cus", [256, 304, 64])
def test_the_shapes_reach_their_regimes(n_cus):
    """Every shape function asserts the regime it names; here for the MI355X's 256 CUs and two other device sizes, with
    the figures the module docstring and DESIGN.md quote for 256."""
    r = regimes(n_cus)
    assert len(r) == 7 + 2 * len(NARROW_BANDS) + len(RAIN_NARROW_BANDS) + 1 == 15
    places, counts = places_for(verify_shape("A", n_cus))
    assert counts[ROLES["three"]] == 3 and counts[ROLES["two"]] == 2 and len(places[ROLES["tail"]]) == 1
    places, counts = places_for(verify_shape("B", n_cus))
    assert ROLES["three"] not in places and counts[ROLES["tail"]] == 2 and counts[ROLES["tail_late"]] == 1
    if n_cus == 256:
        a, b = verify_shape("A", 256), verify_shape("B", 256)
        assert (a.H, a.grid, a.trips) == (8078, 1024, 2052) and (b.H, b.grid, b.n_tail) == (17750, 1024, 266250)
        assert (hist_shape("17", 256).rows, hist_shape("4100", 256).rows) == (8201, 4101)
        f = finish_shape(256)
        assert (f.n_cells, f.n_shared, f.grid) == (116523, 58260, 4096)
        g = bands_shape(256)
        assert (g.rows, g.band_rows, g.bands, g.unweighted_band_rows) == (723, 20, 37, 16)
        assert copy_shape(256).nbytes == 16 * (8199 * 512 + 300)
        n = [narrow_bands_shape(256, wt, b) for wt in (False, True) for b in NARROW_BANDS]
        assert [(v.rows, v.band_rows) for v in n] == [(32785, 17), (524545, 256), (10929, 17), (174849, 256)]
        # and what no short test reaches: bands of 256 rows at this width
        assert band_rows(36001, 255 * 38, 6, 256) == 255 and 36001 * (255 * 38 + 1) > 348000000
        # the rain sums: a block's owned rows in one call (host/grid.c) are items of 127 rows, all of them, ...
        assert ceil_div(36000, RAIN_ITEM_COLS) == 71 and grid_cap(256, RAIN_PER_CU) // 71 + 1 == 58
        assert rain_band_rows(36000, 36000, 256) == RAIN_ITEM_ROWS
        # ... every strip of tests/test_gpu_grid_rain.py stays at the floor, ...
        small = ((1043, 61), (4099, 300), (301, 301), (2100, 24), (17, 17))
        assert [rain_band_rows(w, h, 256) for w, h in small] == [RAIN_FLOOR] * 5
        # ... and the strips of this module do not
        n = [rain_narrow_shape(256, b) for b in RAIN_NARROW_BANDS]
        assert [(v.rows, v.band_rows, v.bands) for v in n] == [(65553, 17, 3857), (516223, 127, 4065), (520320, 127, 4098)]
        f = rain_full_item_shape(256)
        assert (f.want, f.rows, f.W * f.rows, f.bands, f.rows - (f.bands - 1) * f.band_rows) == \
            (2049, 258175, 136316400, 2033, 111)
        assert f.rows_clamp == 260224
