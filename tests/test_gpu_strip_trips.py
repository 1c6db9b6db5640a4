"""GPU: all 78 instantiations of cn_strip_kernel run past their first trip, in both soil forms, and cn_strip_bytes past
its first sweep.  Needs an MI355X (all tests but two, which are arithmetic and run anywhere).

cn_strip_kernel (gcn10_strip.hip) holds three trip loops: strips of any width read the soil code bytes in chunks of
4096 px dealt by first_chunk (kSoilBytes: every real block, 36001 px wide, runs this one), strips of 16-byte aligned rows
keep each lane in one column group (kSoilLanes, and kSoilPixels for a tile with a complex group; strip_lane_plan).  The
grid is capped at grid_blocks_per_cu workgroups per CU, a multiple of 8; beyond the cap a workgroup makes several trips,
and the pipelined variants (PF) then alternate between two register sets.  tests/test_gpu_strip_choice.py launches
every instantiation, on 3 rows: one trip.  The earlier tests of several trips read the soil tables, with NT = true and
condition mask 3 for all but the single-table kernel; of the code bytes only test_too_few_threads_for_one_row
(tests/test_gpu_column_lanes.py) goes round again, with two kernels, and its W % 16 == 0 has no straddling lane.
This module computes each strip's height from the device's CU count with the
launch arithmetic of the sources, restated below beside the constant it mirrors, asserts from that arithmetic that the
strip reaches the regime it names -- the set of trips per workgroup, the trips per piece of the lane plan, the sweeps
of the byte kernel --, asserts the soil state and the kernel's name (the line of tests/golden/strip_kernel_choice.txt:
a request's kernel depends neither on the shape nor on the soil form), and compares every selected raster byte for
byte with the oracle inside poisoned guards (run_strip of tests/test_gpu_column_lanes.py).  No tolerance anywhere.

The regimes of first_chunk, with C = the cap at one workgroup per CU and N = the groups of ILP chunks:
    N = C + 1       slabs     trips {0, 1, 2}: workgroups of the last XCD have nothing to do and leave at trip >= end
    N = C + C / 2   on, off   trips {1, 2}
    N = 3 C + C / 4 on, off   trips {3, 4}
{1, 2} and {3, 4} together take every exit of the PF loop: both breaks, each before and after `ta` is issued again.

A strip that starts inside the tile starts at row 16, not 17: at W = 1043 the landcover pointer of row 17 is not 16-byte
aligned (17 x 1043 = 17731), and such a strip goes to cn_strip_bytes, which is section 5's subject.
"""
import re
import types

import numpy as np
import pytest

from oracle import cn_oracle_c as oc
from tests import soil_readers as sr
from tests.test_gpu_column_lanes import SUBSET, run_strip
from tests.test_gpu_soil_tables import _with_complex_group
from tests.test_gpu_strip_choice import TABLE_MASKS, key_of, read_golden, vector_requests
from tests.test_strip_lane_plan import _run as run_walker
from tests.test_strip_lane_plan import walker  # noqa: F401  (the fixture: tests/strip_lane_plan_main.cpp, compiled)

on_gpu = pytest.mark.gpu
GUARD, POISON = sr.GUARD, 0xA5
ONE, TWO, ALL = TABLE_MASKS
REQUESTS = list(vector_requests())     # the 108 of tests/test_gpu_strip_choice.py, one test each: see profiles/strip_trips


def id_of(q):
    return "cond%d-%s-nt%d-pf%d-ilp%d" % (q["cond"], {ONE: "one", TWO: "two", ALL: "all"}[q["table"]], q["nt"], q["pf"],
                                         q["ilp"])


# ---- the launch arithmetic of the sources ------------------------------------------------------------------------
THREADS = 256               # kThreads (gcn10_device_util.hpp); kStripThreads (gcn10_strip_lanes.hpp)
PX_PER_LANE = 16            # kPxPerLane
CHUNK = THREADS * PX_PER_LANE       # kChunk: 4096 px per workgroup step
WAVE_PX = 64 * PX_PER_LANE          # kWavePx (gcn10_strip.hip)
MIN_VECTOR_W = WAVE_PX + 16         # kMinVectorW: the narrowest strip of the vector kernels
XCDS = 8                    # first_chunk, strip_lane_plan: one slab, one piece per XCD
PER_CU = 1                  # the grid_blocks_per_cu of every launch here
W_BYTES, W_LANES, W_BLOCK, W_ODD = 1043, 1040, 36001, 1039
Y0 = 16                     # the row a strip inside the tile starts at (module docstring)


def ceil_div(a, b):
    return -(-a // b)


def stream_grid(cus, nchunks, per_cu=PER_CU):
    """gcn10_context.hip stream_grid: the cap is rounded down to a multiple of 8 (one slab per XCD), 8 at least"""
    cap = cus * per_cu
    cap = max(cap - cap % XCDS, XCDS)
    return max(min(nchunks, cap), 1)


def cap_of(cus):
    return stream_grid(cus, 1 << 40)


def deal(n, nb, slabs):
    """first_chunk of gcn10_device_util.hpp and the loop `for (; trip < end; trip += step)`: the groups of every
    workgroup.  Slabs apply only when nb % 8 == 0 and nchunks >= nb."""
    out = []
    for b in range(nb):
        if slabs and nb % XCDS == 0 and n >= nb:
            per = ceil_div(n, XCDS)
            lo = (b & 7) * per
            hi = min(lo + per, n)
            out.append(range(lo + (b >> 3), hi, nb // XCDS))
        else:
            out.append(range(b, n, nb))
    return out


def trip_set(n, nb, slabs):
    return {len(r) for r in deal(n, nb, slabs)}


def groups_of(W, rows, ilp):
    """gcn10_gpu_cn_strip: p.nchunks, N = ceil(ceil(npix / 4096) / ILP)"""
    return ceil_div(ceil_div(W * rows, CHUNK), ilp)


def ilp_of(q):
    """gcn10_gpu_cn_strip: ilp1 for one table; else ilp16, where 0 is two sub-chunks up to nine store streams, one
    beyond"""
    n_tables = bin(q["table"]).count("1")
    if n_tables == 1:
        return q.get("ilp", 2)
    ilp = q.get("ilp", 0)
    return ilp if ilp > 0 else (1 if bin(q["cond"]).count("1") * n_tables > 9 else 2)


def name_args(name):
    """(KIND, COND_MASK, ALL_TABLES, ILP, NT, PF) of a kernel's name"""
    m = re.fullmatch(r"cn_strip_kernel<(\d), (\d), (true|false), (\d), (true|false), (true|false)>", name)
    assert m, name
    return tuple(int(v) if v.isdigit() else v == "true" for v in m.groups())


# N as a function of the cap, and the trips per workgroup the regime is named for
REGIMES = {"0-1-2": (lambda c: c + 1, {0, 1, 2}), "1-2": (lambda c: c + c // 2, {1, 2}),
           "3-4": (lambda c: 3 * c + c // 4, {3, 4})}


def bytes_shape(cus, W, ilp, regime, slabs, odd=False):
    """The strip of width W whose groups of `ilp` chunks reach `regime` on a device of `cus` CUs: the fewest rows from
    the regime's N on whose trips per workgroup are the regime's set (W < 4096: N itself).  odd: an odd number of rows."""
    cap = cap_of(cus)
    target, want = REGIMES[regime][0](cap), REGIMES[regime][1]
    first = ceil_div((target - 1) * ilp * CHUNK + 1, W)                 # the fewest rows with N >= target
    s = None
    for rows in range(first, first + 40):
        n = groups_of(W, rows, ilp)
        if (odd and rows % 2 == 0) or trip_set(n, stream_grid(cus, n), slabs) != want:
            continue
        s = types.SimpleNamespace(W=W, ilp=ilp, regime=regime, slabs=slabs, rows=rows, N=n, grid=stream_grid(cus, n))
        break
    assert s is not None, "no strip of W=%d reaches %s at %d CUs" % (W, regime, cus)
    s.npix = W * s.rows
    assert W >= MIN_VECTOR_W and s.npix < 1 << 31 and s.N >= target and (W >= CHUNK or odd or s.N == target)
    assert s.grid == cap and s.grid % XCDS == 0 and s.N >= s.grid          # the cap; slabs apply when asked for
    s.trips = trip_set(s.N, s.grid, slabs)
    assert s.trips == want
    if slabs:
        # the slabs are what deals: workgroup 8 takes group 1 of slab 0, not group 8
        assert list(deal(s.N, s.grid, 1)[8])[0] == 1 and list(deal(s.N, s.grid, 0)[8])[0] == 8
    if regime == "0-1-2":
        idle = [b for b, r in enumerate(deal(s.N, s.grid, slabs)) if len(r) == 0]
        assert idle and all(b & 7 == 7 for b in idle)                   # the idle workgroups are of the last XCD
    if odd:
        # the byte tail behind the loop, and a last wave that is partly dead
        assert s.npix % 16 != 0 and (s.npix & ~15) % WAVE_PX != 0
    s.text = "W=%d ILP %d rows=%d: N=%d over %d workgroups, slabs %d, trips %s" % (
        W, ilp, s.rows, s.N, s.grid, slabs, sorted(s.trips))
    return s


def lane_rows(T, G):
    """gcn10_strip_lanes.hpp strip_lane_rows"""
    B = T // G
    m = 8 if G & 1 else 4 if G & 2 else 2 if G & 4 else 1
    Ba = B - B % m
    return Ba if Ba > 0 and (T - Ba * G) * 20 < T else B


def lane_plan(W, rows, grid, slabs, ilp):
    """gcn10_strip_lanes.hpp strip_lane_plan, for every piece: held to the walker program in
    test_the_shapes_reach_their_regimes"""
    p = types.SimpleNamespace(G=W // 16, pieces=1, T=grid * THREADS)
    if slabs and grid % XCDS == 0 and (grid // XCDS) * THREADS >= p.G:
        p.pieces, p.T = XCDS, (grid // XCDS) * THREADS
    p.B = lane_rows(p.T, p.G)
    p.piece_rows = [(k + 1) * rows // p.pieces - k * rows // p.pieces for k in range(p.pieces)]
    p.trips = [ceil_div(r, p.B * ilp) if p.B else 0 for r in p.piece_rows]
    return p


def lane_shape(cus, W, ilp, k):
    """The strip of 16-byte aligned rows whose pieces take k trips each with a ragged last one: slabs on for k = 3 and
    4, off for 1 and 2.  The plan depends on the grid and the grid on the rows: from the plan at the cap, the fewest
    rows above (k - 1) full trips of every piece that give k trips at the cap (k = 1: the most rows of one trip)."""
    cap, slabs = cap_of(cus), int(k >= 3)
    at_cap = lane_plan(W, 1, cap, slabs, ilp)
    per = at_cap.B * ilp * at_cap.pieces
    rows_to_try = range(per - 1, 0, -1) if k == 1 else range((k - 1) * per + 3 * at_cap.pieces + 5, k * per)
    s = None
    for rows in rows_to_try:
        grid = stream_grid(cus, groups_of(W, rows, ilp))
        p = lane_plan(W, rows, grid, slabs, ilp)
        if p.B and set(p.trips) == {k} and all(r % (p.B * ilp) for r in p.piece_rows) and (k == 1 or grid == cap):
            s = types.SimpleNamespace(W=W, ilp=ilp, k=k, slabs=slabs, rows=rows, grid=grid, plan=p)
            break
    assert s is not None, "no strip of W=%d has %d trips per piece at %d CUs" % (W, k, cus)
    assert W % 16 == 0 and W >= MIN_VECTOR_W and s.plan.B > 0 and s.plan.pieces == (XCDS if slabs else 1)
    assert set(s.plan.trips) == {k} and W * s.rows < 1 << 31
    last = [r - (k - 1) * s.plan.B * ilp for r in s.plan.piece_rows]
    assert all(0 < r < s.plan.B * ilp for r in last)                      # ragged: the last trip is cut in every piece
    s.case = (W, s.rows, s.grid, slabs, ilp)
    s.text = "W=%d ILP %d rows=%d: %d workgroups, %d piece(s), B=%d, %d trips per piece, %s rows in the last" % (
        W, ilp, s.rows, s.grid, s.plan.pieces, s.plan.B, k, sorted(set(last)))
    return s


def sweep_shape(cus, W):
    """cn_strip_bytes: grid = stream_grid(ceil(npix / 256)) and `for (i = ...; i < npix; i += gridDim.x * 256)`: the
    fewest rows of three sweeps with a partly dead last one"""
    cap = cap_of(cus)
    s = types.SimpleNamespace(W=W, sweep=cap * THREADS)
    s.rows = ceil_div(2 * s.sweep + 1, W)
    s.npix = W * s.rows
    s.grid = stream_grid(cus, ceil_div(s.npix, THREADS))
    s.sweeps = ceil_div(s.npix, s.grid * THREADS)
    assert s.grid == cap and s.sweeps >= 3 and s.npix % (s.grid * THREADS) != 0
    s.text = "W=%d rows=%d: %d pixels in %d sweeps of %d" % (W, s.rows, s.npix, s.sweeps, s.grid * THREADS)
    return s


BODIES = [dict(cond=3, table=ALL, ilp=1), dict(cond=3, table=ALL, ilp=2), dict(cond=3, table=TWO, ilp=1),
          dict(cond=3, table=TWO, ilp=2), dict(cond=3, table=ONE, ilp=1), dict(cond=3, table=ONE, ilp=2)]
# section 4: default options but for the ones named (ilp16 = 0: by the number of store streams)
OTHER_WAYS = [dict(cond=3, table=ALL), dict(cond=1, table=ONE, ilp=2), dict(cond=1, table=ONE, ilp=4),
              dict(cond=2, table=TWO)]


def extra_shapes(cus, ilp):
    """the three further launches of a pipelined body: idle workgroups, a strip inside the tile, a byte tail"""
    return [(bytes_shape(cus, W_BYTES, ilp, "0-1-2", 1), 0), (bytes_shape(cus, W_BYTES, ilp, "3-4", 1), Y0),
            (bytes_shape(cus, W_BYTES, ilp, "1-2", 1, odd=True), 0)]


def all_shapes(cus):
    """(the strips of the code bytes, the strips of the lane plan, the strips of the byte kernel) that this module
    launches on a device of `cus` CUs; every shape function asserts its own regime"""
    code_bytes, lanes = [], []
    for ilp in (1, 2, 4):
        code_bytes += [bytes_shape(cus, W_BYTES, ilp, "3-4", 1), bytes_shape(cus, W_BYTES, ilp, "1-2", 0)]
        code_bytes += [bytes_shape(cus, W, ilp, "3-4", 1) for W in (W_BLOCK, W_LANES)]
        lanes += [lane_shape(cus, W_LANES, ilp, k) for k in (1, 2, 3, 4)]
    for ilp in (1, 2):
        code_bytes += [s for s, _y0 in extra_shapes(cus, ilp)]
    return code_bytes, lanes, [sweep_shape(cus, W_ODD), sweep_shape(cus, W_LANES)]


def tile_rows(cus, name):
    """the rows of the module's tile `name`: what its tallest strip needs"""
    code_bytes, lanes, sweeps = all_shapes(cus)
    if name == "1043":
        return max(s.rows for s in code_bytes if s.W == W_BYTES) + Y0
    if name == "36001":
        return max(s.rows for s in code_bytes if s.W == W_BLOCK)
    if name == "1039":
        return sweeps[0].rows
    if name == "1040-complex":
        return max(s.rows for s in lanes if s.k == 3)
    return max([s.rows for s in lanes] + [s.rows for s in code_bytes if s.W == W_LANES] + [sweeps[1].rows])


def short_rows(cus, name):
    """the rows of tile `name` that strips of one or two chunks per trip need: four chunks are for one table only"""
    code_bytes, lanes, sweeps = all_shapes(cus)
    W = TILES[name][0]
    shapes = [s for s in code_bytes + lanes if s.W == W and s.ilp <= 2 and (name == "1040" or getattr(s, "k", 3) == 3)]
    return min(max([s.rows for s in shapes + sweeps if s.W == W]) + Y0, tile_rows(cus, name))


TILES = {"1043": (W_BYTES, 42), "36001": (W_BLOCK, 1441), "1039": (W_ODD, 42), "1040": (W_LANES, 42),
         "1040-complex": (W_LANES, 42)}
ONE_K = 2                   # the table of ONE


class TripTile(sr.ReaderTile):
    """A ReaderTile whose oracle rasters stop where the strips that select them do: all rows for the table of ONE, the
    rows of the strips of one or two chunks per trip for the others."""

    def __init__(self, eng, tables, short, **kw):
        super().__init__(eng, tables, **kw)
        self.short = short

    def rows_of(self, r):
        return self.H if r % 9 == ONE_K else self.short

    def want(self, r):
        if r not in self._want:
            c, n = r // 9, self.rows_of(r)
            if c not in self._soil:
                self._soil[c] = oc.modify_hysogs_data(self.soil, c == 0)
            self._want[r] = oc.calculate_cn(self.esa[:n], self._soil[c][:n], self.tables[r % 9]).reshape(n, self.W)
        return self._want[r]


# ---- 1. the arithmetic, without a GPU ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n_cus", [256, 304, 64])
def test_the_shapes_reach_their_regimes(walker, n_cus):  # noqa: F811
    """Every shape function asserts the regime it names; here for the MI355X's 256 CUs and two other device sizes.  And:
    first_chunk deals every group to exactly one workgroup, with slabs and without; the lane plans are the ones of
    gcn10::strip_lane_plan itself (the walker program, which also visits every vector once)."""
    code_bytes, lanes, sweeps = all_shapes(n_cus)
    assert len(code_bytes) == 3 * 4 + 2 * 3 and len(lanes) == 12 and len(sweeps) == 2
    for s in code_bytes:
        for slabs in (0, 1):
            dealt = sorted(g for r in deal(s.N, s.grid, slabs) for g in r)
            assert dealt == list(range(s.N)), "%s: slabs %d deal a group twice or not at all" % (s.text, slabs)
    # the regimes of the table in the module docstring, at N itself, slabs on and off
    cap = cap_of(n_cus)
    assert trip_set(cap + 1, cap, 1) == {0, 1, 2}
    assert trip_set(cap + cap // 2, cap, 1) == trip_set(cap + cap // 2, cap, 0) == {1, 2}
    assert trip_set(3 * cap + cap // 4, cap, 1) == trip_set(3 * cap + cap // 4, cap, 0) == {3, 4}
    got = run_walker(walker, [s.case for s in lanes])
    for s in lanes:
        assert got[s.case] == dict(pieces=s.plan.pieces, B=s.plan.B, trips=s.k), s.text
    assert (Y0 + 1) * W_BYTES % 16 != 0 and Y0 * W_BYTES % 16 == 0         # row 17 is not aligned, row 16 is
    for name in TILES:
        assert tile_rows(n_cus, name) > 0
    if n_cus == 256:
        assert cap == 256
        s = bytes_shape(256, W_BYTES, 1, "3-4", 1)
        assert (s.rows, s.N) == (3264, 832) and bytes_shape(256, W_BYTES, 4, "3-4", 1).rows == 13054
        s = bytes_shape(256, W_BYTES, 2, "1-2", 0)
        assert (s.rows, s.N) == (3009, 384) and bytes_shape(256, W_BYTES, 1, "0-1-2", 1).N == 257
        s = bytes_shape(256, W_BLOCK, 1, "3-4", 1)
        assert (s.rows, s.N) == (95, 835)                               # the production width: about 95 rows
        assert [(s.rows, s.plan.pieces, s.plan.B) for s in lanes[:4]] == [(1007, 1, 1008), (1016, 1, 1008),
                                                                          (1949, 8, 120), (2909, 8, 120)]
        assert lanes[-1].rows == 11549 and [(s.rows, s.sweeps) for s in sweeps] == [(127, 3), (127, 3)]
        assert {n: tile_rows(256, n) for n in TILES} == {"1043": 13070, "36001": 379, "1039": 127, "1040": 13092,
                                                         "1040-complex": 7709}


def test_the_requests_name_all_78_kernels_with_the_ilp_restated_here():
    """The 108 requests launch, between them, every instantiation: so does a module that launches all 108.  And the
    chunks per trip that the heights are computed from are the ones in the kernel's name."""
    golden = read_golden()
    names = set()
    for q in vector_requests():
        name = golden[key_of(q)]
        kind, cond, _all_tables, ilp, nt, pf = name_args(name)
        single = bin(q["table"]).count("1") == 1
        assert (kind, cond, ilp, nt, pf) == (int(single), q["cond"], ilp_of(q), bool(q["nt"]), bool(q["pf"]) and ilp <= 2)
        names.add(name)
    assert len(names) == 78
    # the six pipelined bodies and the launches of section 4 are requests of the table too
    for q in BODIES:
        assert name_args(golden[key_of(dict(q, tile="1040"))])[3:] == (q["ilp"], True, True)
    for q in OTHER_WAYS:
        for pf in (0, 1):
            assert name_args(golden[key_of(dict(q, tile="1040", pf=pf))])[3] == ilp_of(q)


# ---- the launches -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cus(engine):
    n = engine.device_info()["cus"]
    code_bytes, lanes, sweeps = all_shapes(n)
    print("strips at %d CUs:\n%s" % (n, "\n".join(s.text for s in code_bytes + lanes + sweeps)))
    return n


def make_tile(engine, tables, cus, name):
    """The module's tile `name`, its oracle rasters computed: the strips are cut from its first rows."""
    W, hsx = TILES[name]
    H = tile_rows(cus, name)
    ci = _with_complex_group(W, hsx, 7) if name.endswith("complex") else None
    t = TripTile(engine, tables, short_rows(cus, name), seed=W + len(name), W=W, H=H, hsx=hsx, hsy=H // 25 + 2, ci=ci)
    for r in range(18):
        t.want(r)
    return t


def tile_fixture(name):
    @pytest.fixture(scope="module")
    def tile(engine, tables, cus):
        t = make_tile(engine, tables, cus, name)
        yield t
        engine.sync()
        t.close()
        engine.set_option("defaults", 0)
    return tile


tile_1043, tile_1040, tile_complex = tile_fixture("1043"), tile_fixture("1040"), tile_fixture("1040-complex")
tile_36001, tile_1039 = tile_fixture("36001"), tile_fixture("1039")


@pytest.fixture
def eng9(engine, tables):
    engine.set_tables(tables)
    engine.set_option("defaults", 0)
    yield engine
    engine.set_option("defaults", 0)


def set_request(eng, q, slabs, compact=1):
    """the options of request q on one workgroup per CU; the options it does not name are the defaults"""
    single = bin(q["table"]).count("1") == 1
    eng.set_option("defaults", 0)
    eng.set_option("grid_blocks_per_cu", PER_CU)
    eng.set_option("xcd_slabs", slabs)
    eng.set_option("nontemporal", q.get("nt", 1))
    eng.set_option("prefetch", q.get("pf", 1))
    eng.set_option("compact_soil", compact)
    if "ilp" in q:
        eng.set_option("ilp1" if single else "ilp16", q["ilp"])


def launch(t, q, s, golden, y0=0, compact=1):
    """request q over the strip s of tile t: every selected raster against the oracle, the golden name"""
    key = key_of(dict(q, tile="1040"))
    want = golden[key]
    assert name_args(want)[3] == s.ilp == ilp_of(q) and s.W == t.W
    assert all(y0 + s.rows <= t.rows_of(r) for r in sr.selected(q["cond"], q["table"]))
    set_request(t.eng, q, s.slabs, compact)
    name = run_strip(t, q["cond"], q["table"], "%s; %s" % (key, s.text), y0=y0, rows=s.rows, kernel=want)
    assert name == want, key


# ---- 2. kSoilBytes, every instantiation -------------------------------------------------------------------------------

@on_gpu
@pytest.mark.parametrize("q", REQUESTS, ids=id_of)
def test_code_bytes_on_several_trips(eng9, tile_1043, cus, q):
    """W = 1043: a row end in nearly every wave, a straddling lane at nearly every row end.  The request on trips
    {3, 4} with slabs and on {1, 2} without."""
    t = tile_1043
    t.prepare()
    assert t.W & 15 and eng9.soil_words_state() == 1           # the tile has the tables; W & 15 sends strips to the bytes
    golden = read_golden()
    for regime, slabs in (("3-4", 1), ("1-2", 0)):
        launch(t, q, bytes_shape(cus, t.W, ilp_of(q), regime, slabs), golden)


@on_gpu
@pytest.mark.parametrize("q", BODIES, ids=["all-1", "all-2", "two-1", "two-2", "one-1", "one-2"])
def test_code_bytes_idle_workgroups_inner_strip_and_byte_tail(eng9, tile_1043, cus, q):
    """Each pipelined (KIND, ALL_TABLES, ILP) body: trips {0, 1, 2} with workgroups that leave at once, the {3, 4} strip
    at row 16 of the tile, and an odd number of rows (the byte tail behind the loop, a partly dead last wave)."""
    t = tile_1043
    t.prepare()
    assert t.W & 15 and eng9.soil_words_state() == 1
    golden = read_golden()
    for s, y0 in extra_shapes(cus, q["ilp"]):
        assert y0 * t.W % 16 == 0 and y0 + s.rows <= t.H
        launch(t, q, s, golden, y0=y0)


# ---- 3. kSoilLanes, every instantiation; kSoilPixels ------------------------------------------------------------------

@on_gpu
@pytest.mark.parametrize("q", REQUESTS, ids=id_of)
def test_column_lanes_on_one_to_four_trips(eng9, tile_1040, cus, q):
    """W = 1040 from the compact words: the request on 4 and 3 trips per piece with slabs (eight pieces), on 2 and 1
    without (one piece), the last trip ragged."""
    t = tile_1040
    t.prepare()
    assert eng9.soil_words_state() == 1
    golden = read_golden()
    for k in (4, 3, 2, 1):
        launch(t, q, lane_shape(cus, t.W, ilp_of(q), k), golden)


@on_gpu
@pytest.mark.parametrize("q", [q for q in REQUESTS if q["cond"] == 3 and q["table"] in (ONE, ALL)], ids=id_of)
def test_complex_tile_on_three_trips(eng9, tile_complex, cus, q):
    """kSoilPixels: a tile with a complex group goes pixel by pixel through the codes table, on the same lane plan."""
    t = tile_complex
    t.prepare()
    assert eng9.soil_words_state() == 2
    launch(t, q, lane_shape(cus, t.W, ilp_of(q), 3), read_golden())


# ---- 4. the other ways into kSoilBytes --------------------------------------------------------------------------------

def other_ways(t, cus, q, compact):
    assert t.eng.soil_words_state() == 1 and (t.W & 15 != 0) == (compact == 1)
    golden = read_golden()
    for pf in (0, 1):
        launch(t, dict(q, pf=pf), bytes_shape(cus, t.W, ilp_of(q), "3-4", 1), golden, compact=compact)
        assert t.eng.soil_words_state() == compact


OTHER_IDS = ["cond3-all", "cond1-one-ilp2", "cond1-one-ilp4", "cond2-two"]


@on_gpu
@pytest.mark.parametrize("q", OTHER_WAYS, ids=OTHER_IDS)
def test_block_width_on_several_trips(eng9, tile_36001, cus, q):
    """The production width (W & 15, 8.8 chunks per row) on trips {3, 4}, with the default options but for the ones
    the request names and the pipeline, off and on."""
    tile_36001.prepare()
    other_ways(tile_36001, cus, q, 1)


@on_gpu
@pytest.mark.parametrize("q", OTHER_WAYS, ids=OTHER_IDS)
def test_compact_soil_off_on_several_trips(eng9, tile_1040, cus, q):
    """Aligned rows with compact_soil = 0: the code bytes, made for the first such strip, on trips {3, 4}."""
    tile_1040.prepare()
    other_ways(tile_1040, cus, q, 0)


# ---- 5. cn_strip_bytes past its first sweep ---------------------------------------------------------------------------

def run_bytes(t, cond_mask, table_mask, rows, shift, what):
    """run_strip with every raster `shift` bytes off 16-byte alignment"""
    eng, W = t.eng, t.W
    n = W * rows
    sel = sr.selected(cond_mask, table_mask)
    slot = (n + 2 * GUARD + 16 + 255) & ~255
    arena = eng.alloc(len(sel) * slot)
    try:
        eng.memset(arena.ptr, POISON, len(sel) * slot)
        ptrs = [None] * 18
        for i, r in enumerate(sel):
            ptrs[r] = arena.at(i * slot + GUARD + shift)
        eng.cn_strip(t.bufs[0].ptr, W, rows, t.bufs[3].ptr, cond_mask, table_mask, ptrs)
        name = eng.last_kernel_name()
        img = eng.download(arena.ptr, (len(sel), slot))
    finally:
        eng.sync()
        arena.close()
    assert name == "cn_strip_bytes", "%s: ran %s" % (what, name)
    at = GUARD + shift
    for i, r in enumerate(sel):
        bad = np.argwhere(img[i, at:at + n].reshape(rows, W) != t.want(r)[:rows])
        assert bad.size == 0, "%s: raster %d differs in %d pixels, first at (row, column) %s" % (
            what, r, len(bad), tuple(bad[0]))
        assert (img[i, :at] == POISON).all() and (img[i, at + n:] == POISON).all(), \
            "%s: raster %d wrote outside its pixels" % (what, r)


def byte_kernel(t, cus, shift):
    s = sweep_shape(cus, t.W)
    assert s.rows <= min(t.H, t.short) and (t.W < MIN_VECTOR_W or shift % 16 != 0)
    t.prepare()
    t.eng.set_option("grid_blocks_per_cu", PER_CU)
    for cond in (1, 3):
        for table in (ALL, SUBSET):
            run_bytes(t, cond, table, s.rows, shift, "condition mask %d, tables %#x; %s" % (cond, table, s.text))


@on_gpu
def test_byte_kernel_on_three_sweeps(eng9, tile_1039, cus):
    """W = 1039, below kMinVectorW: the grid-stride loop comes round twice, the last sweep is partly dead."""
    byte_kernel(tile_1039, cus, 0)


@on_gpu
def test_byte_kernel_on_three_sweeps_into_unaligned_rasters(eng9, tile_1040, cus):
    """W = 1040 with every raster one byte off 16-byte alignment."""
    byte_kernel(tile_1040, cus, 1)
