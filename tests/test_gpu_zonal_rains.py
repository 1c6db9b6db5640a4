"""GPU: the words {s, n, sw_1 .. sw_k} per zone with a tuple of weight tables per item (gcn10_gpu_zonal_sums_rains)
through the ABI face, against numpy: the oracle's full-resolution rasters summed over the pixels the spans name, sw_j with
the table that byte j of the item names (a byte >= the number of tables counting as table 0).  Every comparison is bit
for bit; acc always sits inside a poisoned buffer with guards.  The strips, the hand-made pieces and the masks are those
of tests/test_gpu_zonal_rain.py; here a piece carries a tuple, k is 1, 2, 3 and 8, and a zone lies under five tuples that
differ in the last layer only.  Two GPU calls are compared only where their equality is the property: k = 1 against
gcn10_gpu_zonal_sums_rain, two calls against one, garbage in the unused bytes against none."""
import numpy as np
import pytest

from gcn10_amd import gpu, host
from tests import aggutil as au
from tests.test_gpu_zonal_rain import (E_INVAL, E_STATE, GUARD, MASKS, OK, POISON, ROWS, TABLES, Strip, hand_pieces,
                                       scene, strip_inputs)  # noqa: F401
from tests.test_gpu_zonal_rain import plan_of as plan_of_one
from tests.test_gpu_zonal_rain import run_triples as run_triples_one
from tests.util import random_tables

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 8]


def tuple_of(zone, table, k):
    """the tuple of a hand-made piece: layer 0 is the piece's own table (so k = 1 is the one-raster case); zone 4, which
    lies under five tables, gets five tuples that differ in the LAST layer only"""
    t = table & 255
    if zone == 4:
        return [11] * (k - 1) + [t] + [0] * (8 - k)
    return [(t + 37 * j * (1 + zone)) & 255 for j in range(k)] + [0] * (8 - k)


def plan_of(pieces, k):
    """[(zone, table, [(y, x0, x1), ...]), ...] -> (spans, items), one item per piece, in the order given"""
    spans, items = [], []
    for zone, table, sp in pieces:
        items.append((len(spans), len(sp), tuple_of(zone, table, k)))
        spans += [(y, x0, x1, zone) for y, x0, x1 in sp]
    return np.array(spans, host.ZONE_SPAN_DTYPE), np.array(items, host.ZONE_RAINS_ITEM_DTYPE)


def want_words(inp, spans, items, n_zones, k, tables=TABLES, cond_mask=3, table_mask=0x1FF):
    """int64[n_zones][n_sel][2 + k] by the definition"""
    sel = au.selected(cond_mask, table_mask)
    ys, xs, zs, ts = [], [], [], []
    for it in items:
        t = [int(b) if int(b) < len(tables) else 0 for b in it["table"][:k]]
        for s in spans[int(it["first_span"]):int(it["first_span"]) + int(it["n_spans"])]:
            n = int(s["x1"] - s["x0"])
            ys.append(np.full(n, s["y"], np.int64))
            xs.append(np.arange(s["x0"], s["x1"], dtype=np.int64))
            zs.append(np.full(n, s["zone"], np.int64))
            ts.append(np.tile(np.array(t, np.int64)[:, None], (1, n)))
    acc = np.zeros((n_zones, len(sel), 2 + k), np.int64)
    if not ys:
        return acc
    ys, xs, zs = (np.concatenate(a) for a in (ys, xs, zs))
    ts = np.concatenate(ts, axis=1)
    tab = np.asarray(tables, np.int64)
    for q, r in enumerate(sel):
        v = inp.want(r)[ys, xs].astype(np.int64)
        ok = v != 255
        np.add.at(acc[:, q, 0], zs[ok], v[ok])
        np.add.at(acc[:, q, 1], zs[ok], 1)
        for j in range(k):
            np.add.at(acc[:, q, 2 + j], zs[ok], tab[ts[j][ok], v[ok]])
    return acc


def run_words(sc, spans, items, n_zones, k, tables=TABLES, cond_mask=3, table_mask=0x1FF, repeat=1):
    """int64[n_zones][n_sel][2 + k] after set_rain_tables(tables) and `repeat` calls on one zeroed acc; asserts that not
    a byte around the words was written"""
    inp, eng = sc.inp, sc.eng
    n_sel = len(au.selected(cond_mask, table_mask))
    nbytes = n_zones * n_sel * (2 + k) * 8
    buf = eng.alloc(nbytes + 2 * GUARD)
    try:
        eng.set_rain_tables(tables)
        eng.memset(buf.ptr, POISON, nbytes + 2 * GUARD)
        eng.memset(buf.ptr + GUARD, 0, nbytes)
        for _rep in range(repeat):
            eng.zonal_sums_rains(sc.esa_ptr, inp.W, inp.rows, sc.bufs[3].ptr, spans, items, n_zones, cond_mask, table_mask,
                                 k, buf.ptr + GUARD)
        eng.sync()
        img = eng.download(buf.ptr, (nbytes + 2 * GUARD,))
    finally:
        eng.sync()
        buf.close()
    assert (img[:GUARD] == POISON).all() and (img[GUARD + nbytes:] == POISON).all(), "bytes around acc were written"
    return img[GUARD:GUARD + nbytes].view(np.uint64).astype(np.int64).reshape(n_zones, n_sel, 2 + k)


def check(sc, spans, items, n_zones, k, **kw):
    got = run_words(sc, spans, items, n_zones, k, **kw)
    kw.pop("repeat", None)
    want = want_words(sc.inp, spans, items, n_zones, k, **kw)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "W=%d k=%d: %d of %d words differ, first (zone, q, word) = %s: got %d, want %d" % (
        sc.inp.W, k, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    return got


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind", ["shipped", "awkward"])
@pytest.mark.parametrize("W", [1043, 1040])
def test_hand_made_spans_equal_the_summed_oracle(scene, tables, W, kind, k):  # noqa: F811
    lookups = tables if kind == "shipped" else random_tables(41, 9)     # 0, >= 101, 254, 255 and negatives
    sc = scene(strip_inputs((W, kind), W, ROWS, lookups, seed=W + len(kind)))
    spans, items = plan_of(hand_pieces(W, ROWS), k)
    five = np.unique(items["table"][spans["zone"][items["first_span"]] == 4], axis=0)
    assert len(five) == 5 and (five[:, :k - 1] == 11).all()            # five tuples that differ in the last layer only
    for cond_mask, table_mask in MASKS:
        got = check(sc, spans, items, 9, k, cond_mask=cond_mask, table_mask=table_mask)
        assert not got[5].any() and got[..., 1].max() > 0               # zone 5 has no span
    got = check(sc, spans, items, 9, k)
    np.testing.assert_array_equal(got[2, :, :2], got[3, :, :2])        # two zones on the same pixels ...
    assert (got[2, :, 2:] != got[3, :, 2:]).any()                       # ... under other tuples
    assert got[..., 2:].max() > 0 and (got[..., 2 + k - 1] > 0).any()
    # bytes k..7 pick no table: garbage there leaves every word as it is
    if k < 8:
        noisy = items.copy()
        noisy["table"][:, k:] = np.random.default_rng(k).integers(1, 256, (len(items), 8 - k))
        noisy["table"][::2, k:] = 255
        np.testing.assert_array_equal(got, run_words(sc, spans, noisy, 9, k))
    # a byte >= the number of tables counts as table 0: none is with 256 tables, most are with 3
    three = TABLES[[5, 200, 9]]
    assert (items["table"][:, :k] >= 3).any()
    got3 = check(sc, spans, items, 9, k, tables=three)
    clamped = items.copy()
    clamped["table"][:, :k][clamped["table"][:, :k] >= 3] = 0
    np.testing.assert_array_equal(got3, run_words(sc, spans, clamped, 9, k, tables=three))


@pytest.mark.parametrize("k", KS)
def test_two_calls_give_twice_the_words_and_no_items_none(scene, tables, k):  # noqa: F811
    W = 1043
    sc = scene(strip_inputs((W, "shipped"), W, ROWS, tables, seed=W + 7))
    spans, items = plan_of(hand_pieces(W, ROWS), k)
    once = check(sc, spans, items, 9, k)
    np.testing.assert_array_equal(run_words(sc, spans, items, 9, k, repeat=2), 2 * once)
    none = run_words(sc, np.zeros(0, host.ZONE_SPAN_DTYPE), np.zeros(0, host.ZONE_RAINS_ITEM_DTYPE), 9, k)
    assert not none.any()
    # ... and straight through the library, with pointers that would fault if they were read
    rc = gpu.lib().gcn10_gpu_zonal_sums_rains(sc.eng._ctx, None, W, ROWS, None, None, None, 0, 9, 3, 0x1FF, k, None, None)
    assert rc == OK


@pytest.mark.parametrize("W", [1043, 1040])
def test_one_layer_adds_the_words_of_the_one_raster_call(scene, tables, W):  # noqa: F811
    """k = 1: word for word what gcn10_gpu_zonal_sums_rain adds for table = table[0] -- the equality is the property"""
    sc = scene(strip_inputs((W, "shipped"), W, ROWS, tables, seed=W + len("shipped")))
    pieces = [(z, t & 255, sp) for z, t, sp in hand_pieces(W, ROWS)]
    spans, items = plan_of(pieces, 1)
    spans1, items1 = plan_of_one(pieces)
    np.testing.assert_array_equal(spans, spans1)
    np.testing.assert_array_equal(items["table"][:, 0], items1["table"])
    for cond_mask, table_mask in MASKS:
        many = run_words(sc, spans, items, 9, 1, cond_mask=cond_mask, table_mask=table_mask)
        one = run_triples_one(sc, spans1, items1, 9, cond_mask=cond_mask, table_mask=table_mask)
        np.testing.assert_array_equal(many, one)
        assert many.any()


@pytest.mark.parametrize("bounds", [(0, 0), (16, 16), (5, 64)])
def test_spans_cut_by_three_random_fields_equal_the_summed_oracle(scene, tables, bounds):  # noqa: F811
    """The host's own cut (gcn10_zone_rains_cut) of three zones -- the whole strip, a band that shares its pixels, and
    columns 5 .. W - 3 of every third row -- by k = 3 fields of 13 x 7 px cells; the first holds all 256 bytes."""
    W, k = 1043, 3
    sc = scene(strip_inputs((W, "shipped"), W, ROWS, tables, seed=W + 7))
    src = [(y, 0, W, 0) for y in range(ROWS)] + [(y, 100, 900, 1) for y in range(10, 20)] + \
          [(y, 5, W - 3, 2) for y in range(0, ROWS, 3)]
    rng = np.random.default_rng(5)
    cellx, celly = (np.arange(W) // 13).astype(np.int32), (np.arange(ROWS) // 7).astype(np.int32)
    fields = rng.integers(0, 256, (k, int(celly.max()) + 1, int(cellx.max()) + 1)).astype(np.uint8)
    fields[0].reshape(-1)[rng.permutation(fields[0].size)[:256]] = np.arange(256, dtype=np.uint8)
    fields[1] = fields[1] // 64 * 60                   # few bytes: tuples that share a layer
    cut = host.zone_rains_cut({"spans": np.array(src, host.ZONE_SPAN_DTYPE)}, W, ROWS,
                              {"cellx": cellx, "celly": celly, "cx0": 0, "cy0": 0}, fields, *bounds)
    assert len(np.unique(cut["items"]["table"][:, 0])) == 256 and (cut["items"]["table"][:, k:] == 0).all()
    got = check(sc, cut["spans"], cut["items"], 3, k)
    # the cut names every pixel of the source once: s and n are those of the uncut spans under any tuple
    whole = want_words(sc.inp, *plan_of([(z, 0, [s[:3] for s in src if s[3] == z]) for z in range(3)], k), 3, k)
    np.testing.assert_array_equal(got[..., :2], whole[..., :2])
    assert cut["rain_pixels"].tolist() == [W * ROWS, 800 * 10, (W - 8) * len(range(0, ROWS, 3))]


def test_a_sum_past_32_bits_in_the_last_layer_equals_the_closed_form(scene, tables):  # noqa: F811
    """1040 x 68 pixels of one landcover class over one soil code, one zone, one tuple whose LAST table has w[v] = 65535:
    sw_k = 70 720 x 65 535 > 2^32 for every raster that has a value there, the layers before it stay small."""
    W, rows, k = 1040, 68, 8
    esa = np.full((rows, W), 40, np.uint8)
    inp = Strip(W, rows, tables, 1, esa=esa, coarse=np.full((8, 8), 2, np.uint8))
    sc = scene(inp)
    values = {r: np.unique(inp.want(r)) for r in range(18)}
    assert all(len(v) == 1 for v in values.values())
    assert [r for r in range(18) if int(values[r][0]) != 255]
    w = np.zeros((3, 256), np.uint16)
    w[1] = 65535
    w[2] = 3
    tup = [0, 2, 2, 0, 2, 0, 2, 1]
    spans = np.array([(y, 0, W, 0) for y in range(rows)], host.ZONE_SPAN_DTYPE)
    items = np.array([(0, rows, tup)], host.ZONE_RAINS_ITEM_DTYPE)
    got = run_words(sc, spans, items, 1, k, tables=w)
    n = W * rows
    assert n == 70720 and n * 65535 > 1 << 32
    for r in range(18):
        v = int(values[r][0])
        want = [n * v, n] + [n * int(w[t][0]) for t in tup] if v != 255 else [0] * (2 + k)
        assert got[0, r].tolist() == want, (r, v)


def test_state_and_argument_errors_write_nothing(tables):
    eng = gpu.Engine(0)
    L = gpu.lib()
    k = 3
    words = 18 * (2 + 8)
    try:
        inp = Strip(32, 4, tables, 3)
        spans = np.array([(1, 3, 20, 0)], host.ZONE_SPAN_DTYPE)
        items = np.array([(0, 1, [1, 2, 3, 0, 0, 0, 0, 0])], host.ZONE_RAINS_ITEM_DTYPE)
        bufs = [eng.upload(a) for a in (inp.esa, inp.coarse, inp.ci, inp.cj, spans, items)]
        acc = eng.alloc(words * 8)
        eng.memset(acc.ptr, 0, words * 8)

        def call(W=32, rows=4, n_zones=1, cond=3, table=0x1FF, k=k, acc_ptr=acc.ptr, sp=bufs[4].ptr, it=bufs[5].ptr,
                 esa=bufs[0].ptr, cj=bufs[3].ptr):
            rc = L.gcn10_gpu_zonal_sums_rains(eng._ctx, esa, W, rows, cj, sp, it, 1, n_zones, cond, table, k, acc_ptr, None)
            return rc, L.gcn10_gpu_last_error().decode()

        def untouched():
            eng.sync()
            return not eng.download(acc.ptr, (words,), np.uint64).any()
        rc, msg = call()
        assert rc == E_STATE and "gcn10_gpu_set_tables" in msg, (rc, msg)
        eng.set_tables(tables)
        rc, msg = call()
        assert rc == E_STATE and "gcn10_gpu_zonal_sums_rains" in msg, (rc, msg)      # no prepared tile, no rain tables
        eng.prepare_tile(bufs[1].ptr, inp.hsx, inp.hsy, bufs[2].ptr, 32)
        rc, msg = call()
        assert rc == E_STATE and "call gcn10_gpu_set_rain_tables first" in msg, (rc, msg)
        assert untouched()
        eng.set_rain_tables(TABLES)
        rc, msg = call(W=48)
        assert rc == E_STATE and "prepare" in msg, (rc, msg)
        for kw in (dict(k=0), dict(k=9), dict(k=-1), dict(rows=0), dict(n_zones=0), dict(cond=0), dict(cond=4),
                   dict(table=0), dict(table=1 << 9), dict(acc_ptr=None), dict(sp=None), dict(it=None), dict(esa=None),
                   dict(cj=None)):
            rc, msg = call(**kw)
            assert rc == E_INVAL and "gcn10_gpu_zonal_sums_rains" in msg, (kw, rc, msg)
        # k outside 1..8 is refused even where there is nothing to do
        rc = L.gcn10_gpu_zonal_sums_rains(eng._ctx, None, 32, 4, None, None, None, 0, 1, 3, 0x1FF, 9, None, None)
        assert rc == E_INVAL
        assert untouched()
        rc, msg = call()
        assert rc == OK, msg
        eng.sync()
        got = eng.download(acc.ptr, (words,), np.uint64)
        assert got[:18 * (2 + k)].any() and not got[18 * (2 + k):].any()
    finally:
        eng.sync()
        eng.close()
