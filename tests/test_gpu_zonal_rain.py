"""GPU: the triples {s, n, sw} per zone with a weight table per item (gcn10_gpu_zonal_sums_rain) through the ABI face,
against numpy: the oracle's full-resolution rasters summed over the pixels the spans name, sw with the table the item
names (an entry >= k counting as table 0).  Every comparison is bit for bit; acc always sits inside a poisoned buffer
with guards.  Shapes are the smallest at which the kernel can go wrong: spans that begin and end inside a 16-pixel
group, spans of one pixel, a span in the row's last partial group, zones that share pixels, a zone under five tables, a
(zone, table) over several items, more items than workgroups, a sum past 32 bits.  Only the equality with
gcn10_gpu_zonal_pair_histogram compares two GPU calls: there the equality is the property."""
import numpy as np
import pytest

from gcn10_amd import gpu, host
from tests import aggutil as au
from tests import rainutil as rn
from tests.test_gpu_aggregate import Scene
from tests.util import ESA_NASTY, HSG_NASTY, random_tables

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_STATE = 0, -1, -4
POISON, GUARD = 0xA5, 64
TABLES = rn.tables_256()
ROWS = 40
PER_CU = 4                  # gcn10_zonal_rain.hip: grid_cap(ctx, 4)
_INPUTS = {}


class Strip:
    """Random landcover over an 8 x 8 soil window (64 cells); what tests.test_gpu_aggregate.Scene takes."""

    def __init__(self, W, rows, tables, seed, esa=None, coarse=None):
        rng = np.random.default_rng(seed)
        self.W, self.rows, self.tables = W, rows, tables
        self.esa = np.ascontiguousarray(rng.choice(ESA_NASTY, size=(rows, W)) if esa is None else esa).astype(np.uint8)
        self.hsx = self.hsy = 8
        self.coarse = (rng.choice(HSG_NASTY, size=(8, 8)) if coarse is None else coarse).astype(np.uint8)
        self.ci = ((np.arange(W) * 8) // W).astype(np.int32)
        self.cj = ((np.arange(rows) * 8) // rows).astype(np.int32)
        self.soil = self.coarse[self.cj[:, None], self.ci[None, :]]
        self._want = {}

    def want(self, r):
        if r not in self._want:
            self._want.update(au.oracle_rasters(self.esa, self.soil, self.tables, [r]))
        return self._want[r]


def strip_inputs(key, W, rows, tables, seed):
    if key not in _INPUTS:
        _INPUTS[key] = Strip(W, rows, tables, seed)
    return _INPUTS[key]


@pytest.fixture
def scene(engine):
    made = []

    def make(inp):
        made.append(Scene(engine, inp, offset=1))
        return made[-1]
    yield make
    for s in made:
        s.close()


def plan_of(pieces):
    """[(zone, table, [(y, x0, x1), ...]), ...] -> (spans, items), one item per piece, in the order given"""
    spans, items = [], []
    for zone, table, sp in pieces:
        items.append((len(spans), len(sp), table, 0))
        spans += [(y, x0, x1, zone) for y, x0, x1 in sp]
    return np.array(spans, host.ZONE_SPAN_DTYPE), np.array(items, host.ZONE_RAIN_ITEM_DTYPE)


def want_triples(inp, spans, items, n_zones, tables=TABLES, cond_mask=3, table_mask=0x1FF):
    """int64[n_zones][n_sel][3] by the definition"""
    sel = au.selected(cond_mask, table_mask)
    ys, xs, zs, ts = [], [], [], []
    for it in items:
        t = int(it["table"]) if int(it["table"]) < len(tables) else 0
        for s in spans[int(it["first_span"]):int(it["first_span"]) + int(it["n_spans"])]:
            n = int(s["x1"] - s["x0"])
            ys.append(np.full(n, s["y"], np.int64))
            xs.append(np.arange(s["x0"], s["x1"], dtype=np.int64))
            zs.append(np.full(n, s["zone"], np.int64))
            ts.append(np.full(n, t, np.int64))
    acc = np.zeros((n_zones, len(sel), 3), np.int64)
    if not ys:
        return acc
    ys, xs, zs, ts = (np.concatenate(a) for a in (ys, xs, zs, ts))
    tab = np.asarray(tables, np.int64)
    for q, r in enumerate(sel):
        v = inp.want(r)[ys, xs].astype(np.int64)
        ok = v != 255
        for k, w in enumerate((v[ok], np.ones(int(ok.sum()), np.int64), tab[ts[ok], v[ok]])):
            np.add.at(acc[:, q, k], zs[ok], w)
    return acc


def run_triples(sc, spans, items, n_zones, tables=TABLES, cond_mask=3, table_mask=0x1FF, repeat=1, rows=None):
    """int64[n_zones][n_sel][3] after set_rain_tables(tables) and `repeat` calls on one zeroed acc; asserts that not a
    byte around the words was written"""
    inp, eng = sc.inp, sc.eng
    n_sel = len(au.selected(cond_mask, table_mask))
    nbytes = n_zones * n_sel * 24
    buf = eng.alloc(nbytes + 2 * GUARD)
    try:
        eng.set_rain_tables(tables)
        eng.memset(buf.ptr, POISON, nbytes + 2 * GUARD)
        eng.memset(buf.ptr + GUARD, 0, nbytes)
        for _rep in range(repeat):
            eng.zonal_sums_rain(sc.esa_ptr, inp.W, inp.rows if rows is None else rows, sc.bufs[3].ptr, spans, items,
                                n_zones, cond_mask, table_mask, buf.ptr + GUARD)
        eng.sync()
        img = eng.download(buf.ptr, (nbytes + 2 * GUARD,))
    finally:
        eng.sync()
        buf.close()
    assert (img[:GUARD] == POISON).all() and (img[GUARD + nbytes:] == POISON).all(), "bytes around acc were written"
    return img[GUARD:GUARD + nbytes].view(np.uint64).astype(np.int64).reshape(n_zones, n_sel, 3)


def check(sc, spans, items, n_zones, **kw):
    got = run_triples(sc, spans, items, n_zones, **kw)
    kw.pop("repeat", None)
    want = want_triples(sc.inp, spans, items, n_zones, **kw)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "W=%d: %d of %d words differ, first (zone, q, word) = %s: got %d, want %d" % (
        sc.inp.W, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    return got


def hand_pieces(W, rows):
    last = rows - 1
    inside = [(3, 17, 22), (5, 3, 45), (9, 0, 6), (9, 9, 40), (10, 15, 17), (11, 33, 47)]       # begin / end inside a group
    ones = [(y, x, x + 1) for y in (0, 7, last) for x in (0, 1, 15, 16, 17, 31, W - 1)]        # one pixel each
    tail = [(last - 1, W - 5, W), (last, W - 20, W), (last, (W - 1) // 16 * 16, W)]            # the row's last group
    block = [(y, 100, 400) for y in range(12, 30)]
    wide = [(y, 0, W) for y in range(20, 26)]
    return [
        (0, 7, inside), (0, 7, ones),                   # one (zone, table) in two items
        (1, 200, tail),
        (2, 9, block), (3, 254, block),                 # two zones naming the same pixels, under two tables
        (4, 0, wide[:1]), (4, 3, wide[1:2]), (4, 7, wide[2:3]), (4, 128, wide[3:4]), (4, 255, wide[4:]),   # 5 tables
        (6, 31, wide[:2]), (6, 31, wide[2:4]), (6, 31, [(25, 0, 17), (25, 17, W)]),     # zone 5 has no span
        (7, 300, inside),                               # names no table: table 0
        (8, 1, [(last, W - 1, W)]),                     # the strip's last pixel alone
    ]


MASKS = [(3, 0x1FF), (2, 0x1FF), (1, 1 << 4), (3, 0b101), (2, 1 << 8)]


@pytest.mark.parametrize("kind", ["shipped", "awkward"])
@pytest.mark.parametrize("W", [1043, 1040])
def test_hand_made_spans_equal_the_summed_oracle(scene, tables, W, kind):
    lookups = tables if kind == "shipped" else random_tables(41, 9)     # 0, >= 101, 254, 255 and negatives
    sc = scene(strip_inputs((W, kind), W, ROWS, lookups, seed=W + len(kind)))
    if kind == "awkward":
        values = np.unique(np.concatenate([sc.inp.want(r).reshape(-1) for r in (0, 4, 17)]))
        assert {0, 254, 255} <= set(values.tolist()) and (values[(values > 100) & (values < 254)]).size
    spans, items = plan_of(hand_pieces(W, ROWS))
    for cond_mask, table_mask in MASKS:
        got = check(sc, spans, items, 9, cond_mask=cond_mask, table_mask=table_mask)
        assert not got[5].any() and got[..., 1].max() > 0
    got = check(sc, spans, items, 9)
    np.testing.assert_array_equal(got[2, :, :2], got[3, :, :2])        # the same pixels ...
    assert (got[2, :, 2] != got[3, :, 2]).any()                         # ... under another table
    assert got[..., 2].max() > 0
    # a table >= k counts as table 0
    same = items.copy()
    same["table"][same["table"] == 300] = 0
    np.testing.assert_array_equal(got, run_triples(sc, spans, same, 9))
    three = TABLES[[5, 200, 9]]
    got3 = check(sc, spans, items, 9, tables=three)
    clamped = items.copy()
    clamped["table"][clamped["table"] >= 3] = 0
    np.testing.assert_array_equal(got3, run_triples(sc, spans, clamped, 9, tables=three))


def test_two_calls_give_twice_the_words_and_no_items_none(scene, tables):
    W = 1043
    sc = scene(strip_inputs((W, "shipped"), W, ROWS, tables, seed=W + 7))
    spans, items = plan_of(hand_pieces(W, ROWS))
    once = check(sc, spans, items, 9)
    np.testing.assert_array_equal(run_triples(sc, spans, items, 9, repeat=2), 2 * once)
    none = run_triples(sc, np.zeros(0, host.ZONE_SPAN_DTYPE), np.zeros(0, host.ZONE_RAIN_ITEM_DTYPE), 9)
    assert not none.any()
    # ... and straight through the library, with pointers that would fault if they were read
    rc = gpu.lib().gcn10_gpu_zonal_sums_rain(sc.eng._ctx, None, W, ROWS, None, None, None, 0, 9, 3, 0x1FF, None, None)
    assert rc == OK


@pytest.mark.parametrize("bounds", [(0, 0), (16, 16), (5, 64)])
def test_spans_cut_by_a_random_field_equal_the_summed_oracle(scene, tables, bounds):
    """The host's own cut (gcn10_zone_rain_cut) of three zones -- the whole strip, a band that shares its pixels, and
    columns 5 .. W - 3 of every third row -- by a field of 13 x 7 px cells with all 256 bytes."""
    W = 1043
    sc = scene(strip_inputs((W, "shipped"), W, ROWS, tables, seed=W + 7))
    src = [(y, 0, W, 0) for y in range(ROWS)] + [(y, 100, 900, 1) for y in range(10, 20)] + \
          [(y, 5, W - 3, 2) for y in range(0, ROWS, 3)]
    rng = np.random.default_rng(5)
    cellx, celly = (np.arange(W) // 13).astype(np.int32), (np.arange(ROWS) // 7).astype(np.int32)
    field = rng.integers(0, 256, (int(celly.max()) + 1, int(cellx.max()) + 1)).astype(np.uint8)
    field.reshape(-1)[rng.permutation(field.size)[:256]] = np.arange(256, dtype=np.uint8)
    cut = host.zone_rain_cut({"spans": np.array(src, host.ZONE_SPAN_DTYPE)}, W, ROWS,
                             {"cellx": cellx, "celly": celly, "cx0": 0, "cy0": 0}, field, *bounds)
    assert len(np.unique(cut["items"]["table"])) == 256
    got = check(sc, cut["spans"], cut["items"], 3)
    # the cut names every pixel of the source once: s and n are those of the uncut spans under any table
    whole = want_triples(sc.inp, *plan_of([(z, 0, [s[:3] for s in src if s[3] == z]) for z in range(3)]), 3)
    np.testing.assert_array_equal(got[..., :2], whole[..., :2])
    assert cut["rain_pixels"].tolist() == [W * ROWS, 800 * 10, (W - 8) * len(range(0, ROWS, 3))]


def test_no_rain_tables_is_a_state_error(tables):
    eng = gpu.Engine(0)
    L = gpu.lib()
    try:
        inp = Strip(32, 4, tables, 3)
        spans, items = plan_of([(0, 0, [(1, 3, 20)])])
        bufs = [eng.upload(a) for a in (inp.esa, inp.coarse, inp.ci, inp.cj, spans, items)]
        acc = eng.alloc(18 * 24)
        eng.memset(acc.ptr, 0, 18 * 24)

        def call(W=32, rows=4, n_zones=1, cond=3, table=0x1FF, acc_ptr=acc.ptr, sp=bufs[4].ptr):
            rc = L.gcn10_gpu_zonal_sums_rain(eng._ctx, bufs[0].ptr, W, rows, bufs[3].ptr, sp, bufs[5].ptr, 1, n_zones,
                                             cond, table, acc_ptr, None)
            return rc, L.gcn10_gpu_last_error().decode()
        rc, msg = call()
        assert rc == E_STATE and "gcn10_gpu_set_tables" in msg, (rc, msg)
        eng.set_tables(tables)
        eng.prepare_tile(bufs[1].ptr, inp.hsx, inp.hsy, bufs[2].ptr, 32)
        rc, msg = call()
        assert rc == E_STATE and "call gcn10_gpu_set_rain_tables first" in msg, (rc, msg)
        eng.sync()
        assert not eng.download(acc.ptr, (18 * 3,), np.uint64).any()
        eng.set_rain_tables(TABLES)
        rc, msg = call(W=48)
        assert rc == E_STATE and "prepare" in msg, (rc, msg)
        for kw in (dict(rows=0), dict(n_zones=0), dict(cond=0), dict(cond=4), dict(table=0), dict(table=1 << 9),
                   dict(acc_ptr=None), dict(sp=None)):
            rc, msg = call(**kw)
            assert rc == E_INVAL and "gcn10_gpu_zonal_sums_rain" in msg, (kw, rc, msg)
        rc, msg = call()
        assert rc == OK, msg
        eng.sync()
        assert eng.download(acc.ptr, (18 * 3,), np.uint64).any()
    finally:
        eng.sync()
        eng.close()


def test_a_sum_past_32_bits_equals_the_closed_form(scene, tables):
    """1040 x 68 pixels of one landcover class over one soil code, one zone, one table with w[v] = 65535: sw = 70 720 x
    65 535 > 2^32 for every raster that has a value there."""
    W, rows = 1040, 68
    esa = np.full((rows, W), 40, np.uint8)
    inp = Strip(W, rows, tables, 1, esa=esa, coarse=np.full((8, 8), 2, np.uint8))
    sc = scene(inp)
    values = {r: np.unique(inp.want(r)) for r in range(18)}
    assert all(len(v) == 1 for v in values.values())
    with_value = [r for r in range(18) if int(values[r][0]) != 255]
    assert with_value
    w = np.zeros((2, 256), np.uint16)
    w[1] = 65535
    spans, items = plan_of([(0, 1, [(y, 0, W) for y in range(rows)])])
    got = run_triples(sc, spans, items, 1, tables=w)
    n = W * rows
    assert n == 70720 and n * 65535 > 1 << 32
    for r in range(18):
        v = int(values[r][0])
        want = [n * v, n, n * 65535] if v != 255 else [0, 0, 0]
        assert got[0, r].tolist() == want, (r, v)


def test_more_items_than_twice_the_workgroups(scene, tables, engine):
    """Items of 16 px over every pixel: n_items >= 2 x cap + 1, so every workgroup takes at least two items and the
    (zone, table) changes inside a workgroup's run."""
    W = 1040
    cap = PER_CU * int(engine.device_info()["cus"])
    per_row = W // 16
    rows = -(-(2 * cap + 1) // per_row)
    inp = strip_inputs((W, rows, "cap"), W, rows, tables, seed=rows)
    sc = scene(inp)
    src = np.array([(y, 0, W, y % 37) for y in range(rows)], host.ZONE_SPAN_DTYPE)
    src = src[np.lexsort((src["y"], src["zone"]))]
    cellx, celly = (np.arange(W) // 48).astype(np.int32), (np.arange(rows) // 3).astype(np.int32)
    field = np.random.default_rng(9).integers(0, 256, (int(celly.max()) + 1, int(cellx.max()) + 1)).astype(np.uint8)
    cut = host.zone_rain_cut({"spans": src}, W, rows, {"cellx": cellx, "celly": celly, "cx0": 0, "cy0": 0}, field, 16, 16)
    assert len(cut["items"]) >= 2 * cap + 1
    assert int(cut["rain_pixels"].sum()) == W * rows
    keys = cut["spans"]["zone"][cut["items"]["first_span"]].astype(np.int64) * 256 + cut["items"]["table"]
    per_wg = -(-len(keys) // cap)
    changes = [len(set(keys[a:a + per_wg].tolist())) > 1 for a in range(0, len(keys), per_wg)]
    assert per_wg >= 2 and sum(changes) > len(changes) // 4 and not all(changes)       # runs with and without a change
    check(sc, cut["spans"], cut["items"], 37, cond_mask=1, table_mask=0b11)


def test_a_constant_field_equals_the_host_rule_on_the_pair_histogram(scene, tables, engine):
    """Every pixel inside the raster and one byte everywhere: {s, n} and sw equal what the host derives, with
    gcn10_raster_histogram and the table, from gcn10_gpu_zonal_pair_histogram on the uncut spans."""
    W = 1043
    sc = scene(strip_inputs((W, "shipped"), W, ROWS, tables, seed=W + 7))
    src = np.array([(y, 0, W, 0) for y in range(ROWS)] + [(y, 7, 1000, 1) for y in range(3, 30)], host.ZONE_SPAN_DTYPE)
    b = 20
    cellx, celly = (np.arange(W) // 100).astype(np.int32), (np.arange(ROWS) // 100).astype(np.int32)
    field = np.full((1, int(cellx.max()) + 1), b, np.uint8)
    cut = host.zone_rain_cut({"spans": src}, W, ROWS, {"cellx": cellx, "celly": celly, "cx0": 0, "cy0": 0}, field)
    assert len(cut["spans"]) == len(src) and (cut["items"]["table"] == b).all()
    got = run_triples(sc, cut["spans"], cut["items"], 2)
    s2, items = host.zone_items(src)
    hist = engine.alloc(2 * 4096 * 8)
    try:
        engine.memset(hist.ptr, 0, 2 * 4096 * 8)
        engine.zonal_pair_histogram(sc.esa_ptr, W, ROWS, sc.bufs[3].ptr, s2, items, 2, hist.ptr)
        pair = engine.download(hist.ptr, (2, 4096), np.uint64)
    finally:
        hist.close()
    codes = gpu.pair_histogram_codes()
    values = np.arange(256, dtype=np.int64)
    q = TABLES[b].astype(np.int64)
    for z in range(2):
        for r in range(18):
            h = host.raster_histogram(pair[z], codes, tables[r % 9], r < 9).astype(np.int64)
            h[255] = 0
            assert got[z, r].tolist() == [int((h * values).sum()), int(h.sum()), int((h * q).sum())], (z, r)
