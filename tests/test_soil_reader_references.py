"""CPU: the references of tests/test_gpu_soil_readers.py checked against an independent statement of each -- the
column rule value by value, plain indexing against the oracle's resample loop, the per-zone counts against the pair
histogram of the whole strip -- and the shapes the reader tests rely on."""
import numpy as np
import pytest

from gcn10_amd import host
from oracle import cn_oracle_c as oc
from tests import aggutil
from tests import soil_readers as sr
from tests.test_gpu_stats import model_histogram
from tests.util import ESA_NASTY, HSG_NASTY, make_block


def test_clamp_columns_is_the_unsigned_rule_for_every_value_used():
    """(uint32) ci < hsx ? ci : hsx - 1, in Python integers, for every (value, hsx) of the tiles A to G."""
    seen = 0
    for name, spec in sr.SPECS.items():
        W, hsx = spec["W"], spec["hsx"]
        ci = sr._default_map(W, hsx) if spec["ci"] is None else spec["ci"]
        assert ci.dtype == np.int32 and ci.shape == (W,)
        values = np.unique(ci)
        got = sr.clamp_columns(values, hsx)
        for v, g in zip(values.tolist(), got.tolist()):
            u = v & 0xFFFFFFFF
            assert g == (u if u < hsx else hsx - 1), (name, v)
        seen += len(values)
    assert seen > 500
    for hsx in (1, 64, 90, 3000):
        outside = np.array(sr.OUTSIDE + (hsx, hsx - 1, 0), np.int32)
        want = [v if 0 <= v < hsx else hsx - 1 for v in outside.tolist()]       # negative = huge as unsigned
        assert sr.clamp_columns(outside, hsx).tolist() == want
    # case B really holds every kind of value the issue names
    assert {-1, 64, 2 ** 31 - 1} <= set(sr.outside_map("runs").tolist())
    assert {-1, 64, 2 ** 31 - 1, -2 ** 31} <= set(sr.outside_map("scattered").tolist())


@pytest.mark.parametrize("H,W,hsy,hsx,jitter", [(40, 2048, 6, 90, True), (37, 1003, 5, 41, True), (3, 17, 2, 3, False),
                                                 (270, 300, 13, 14, True)])
def test_plain_indexing_equals_the_oracles_resample(H, W, hsy, hsx, jitter):
    _esa, gt, coarse, sgt = make_block(H + W, H, W, hsy, hsx, nasty=True, jitter=jitter)
    ci, cj = host.build_index_maps(gt, sgt, W, H, hsx, hsy)
    np.testing.assert_array_equal(coarse[cj][:, ci], oc.resample(coarse, gt, sgt, W, H))
    np.testing.assert_array_equal(coarse[cj][:, sr.clamp_columns(ci, hsx)], oc.resample(coarse, gt, sgt, W, H))


@pytest.mark.parametrize("W,H", [(5, 3), (17, 3), (300, 27), (2051, 8)])
def test_zones_that_tile_the_strip_sum_to_the_pair_histogram(W, H):
    rng = np.random.default_rng(W * H)
    esa = rng.choice(ESA_NASTY, size=(H, W)).astype(np.uint8)
    soil = rng.choice(HSG_NASTY, size=(H, W)).astype(np.uint8)
    n_zones, spans = 3, []
    for y in range(H):
        cuts = np.unique(np.concatenate([[0, W], rng.integers(0, W + 1, 4)]))
        for a, b in zip(cuts[:-1], cuts[1:]):
            spans.append((y, int(a), int(b), int(rng.integers(0, n_zones))))
    spans = np.array(spans, host.ZONE_SPAN_DTYPE)
    counts = sr.zone_counts(esa, soil, spans, n_zones)
    np.testing.assert_array_equal(counts.sum(axis=0), model_histogram(esa, soil))
    assert int(counts.sum()) == W * H
    # and the counts of one zone are those of its pixels alone
    only = spans[spans["zone"] == 1]
    mask = np.zeros((H, W), bool)
    for s in only:
        mask[s["y"], s["x0"]:s["x1"]] = True
    np.testing.assert_array_equal(counts[1], np.bincount(sr.pair_keys(esa, soil)[mask], minlength=sr.HIST))


@pytest.mark.parametrize("name", list(sr.SPECS))
def test_the_spans_and_strips_of_the_readers_have_the_shapes_the_cases_name(name):
    spec = sr.SPECS[name]
    W, H = spec["W"], spec["H"]
    sp = sr.reader_spans(W, H)
    assert ((sp["y"] >= 0) & (sp["y"] < H) & (sp["x0"] >= 0) & (sp["x0"] < sp["x1"]) & (sp["x1"] <= W)).all()
    assert set(sp["zone"].tolist()) == {0, 1}
    assert (sp["x0"] == 0).any() and (sp["x1"] == W).any()
    inside = (sp["x0"] % 16 != 0) & (sp["x1"] % 16 != 0) & (sp["x0"] // 16 == (sp["x1"] - 1) // 16)
    assert inside.any(), "no span starts and ends inside one 16-px group"
    cover = np.zeros((H, W), np.int32)               # no pixel is named twice
    for s in sp:
        cover[s["y"], s["x0"]:s["x1"]] += 1
    assert cover.max() == 1
    if W >= 64:                                      # ragged: the edges differ from row to row
        assert len(set(sp["x0"][sp["zone"] == 0].tolist())) > 3 and len(set(sp["x1"][sp["zone"] == 1].tolist())) > 3
    cj = np.minimum((np.arange(H) + 3) * spec["hsy"] // (H + 3), spec["hsy"] - 1)
    strips = sr.strips_inside_a_soil_row(cj)
    assert len(strips) == 2 and strips[0][1] + strips[1][1] == H and cj[strips[1][0]] == cj[strips[1][0] - 1]
    assert cj.min() >= 0 and cj.max() < spec["hsy"]


    # the passes of the aggregate reader
    passes = sr.aggregate_passes(W, cj.astype(np.int32))
    assert [p["f"] for p in passes] == [3, 16, 25] and {p["form"] for p in passes} == {sr.AGG_SMALL, sr.AGG_WIDE}
    for p in passes:
        assert 0 <= p["x0"] < p["x1"] <= W and p["Wa"] >= 1 and p["sel"]
        assert len(p["cell_rows"]) == len(p["strips"]) and min(p["cell_rows"]) >= 1
        assert [y0 for y0, _ in p["strips"]] == np.cumsum([0] + [n for _, n in p["strips"]])[:-1].tolist()
        assert sum(n for _, n in p["strips"]) == H                  # the strips tile the rows, in order
    assert passes[0]["strips"] == strips and passes[2]["strips"] == strips and len(passes[1]["strips"]) == H
    assert (passes[0]["x0"], passes[0]["x1"]) == (0, W) == (passes[1]["x0"], passes[1]["x1"])
    assert len(passes[2]["sel"]) < 18
    if W >= 32:                                      # first and last column inside a 16-px group
        assert passes[2]["x0"] % 16 != 0 and passes[2]["x1"] % 16 != 0
        assert passes[2]["x0"] == 1 and W - 2 <= passes[2]["x1"] <= W - 1

    # the passes of the grid reader
    rows, storms = sr.grid_passes(W, H, cj.astype(np.int32))
    assert (rows["name"], storms["name"]) == ("rows", "storms") and (rows["words"], storms["words"]) == (2, 4)
    for p in (rows, storms):
        assert p["cellx"].dtype == p["celly"].dtype == np.int32 and p["cellx"].shape == (W,) and p["celly"].shape == (H,)
        assert p["cellx"].max() == p["ncx"] - 1 and p["celly"].max() == p["ncy"] - 1
        for m in (p["cellx"], p["celly"]):          # the cells of a map never go back, and a cell column is >= 8 px or
            inside = m[m >= 0]                      # cut by the tile's edge: the kernel's three-masks rule
            assert (np.diff(inside) >= 0).all() and set(inside.tolist()) == set(range(int(m.max()) + 1))
        widths = np.bincount(p["cellx"][p["cellx"] >= 0])
        assert (widths[1:-1] >= 8).all()
        assert sum(n for _, n in p["strips"]) == H and p["strips"][0][0] == 0
    assert (rows["cellx"] >= 0).all() and (rows["celly"] >= 0).all()                    # no -1 entry
    assert np.bincount(rows["cellx"]).max() <= 8 and np.bincount(rows["celly"]).max() == 1
    assert rows["strips"] == [(0, H)] and len(rows["sel"]) == 18 and rows["call"] == "grid_sums"
    (lx, ly), (tx, ty) = sr.grid_edges(W, H)
    assert (lx, tx) == ((5, 3) if W >= 32 else (0, 0)) and (ly, ty) == ((3, 2) if H >= 8 else (0, 0))
    for m, lead, trail in ((storms["cellx"], lx, tx), (storms["celly"], ly, ty)):
        assert np.flatnonzero(m < 0).tolist() == list(range(lead)) + list(range(len(m) - trail, len(m)))
    if W >= 32:                                      # the leading -1 run ends inside a 16-px group
        assert (storms["cellx"][:16] < 0).any() and (storms["cellx"][:16] >= 0).any()
    assert storms["strips"] == strips and storms["call"] == "grid_sums_storms" and len(storms["ws"]) == 2
    y0 = storms["strips"][1][0]
    assert cj[y0] == cj[y0 - 1] and storms["celly"][y0] == storms["celly"][y0 - 1] >= 0    # inside a soil and a cell row
    assert 0 < len(storms["sel"]) < 18
    weighted = sr.weighted_rows_pass(W, H, cj.astype(np.int32))
    assert weighted["words"] == 3 and len(weighted["ws"]) == 1 and weighted["call"] == "grid_sums_weighted"
    assert np.array_equal(weighted["cellx"], rows["cellx"]) and weighted["strips"] == rows["strips"]


# ---- the reference of the aggregate reader ---------------------------------------------------------------------------

def cells_by_hand(raster, x0, x1, f, strips):
    """The cells of the strips in Python integers, cell by cell: (2 s + n) // (2 n) over the values != 255, 255 where
    there is none."""
    v = np.asarray(raster).tolist()
    out = []
    for y0, rows in strips:
        for top in range(y0, y0 + rows, f):
            line = []
            for left in range(x0, x1, f):
                s = n = 0
                for y in range(top, min(top + f, y0 + rows)):
                    for value in v[y][left:min(left + f, x1)]:
                        if value != 255:
                            s, n = s + value, n + 1
                line.append((2 * s + n) // (2 * n) if n else 255)
            out.append(line)
    return out


def check_reduction(rasters, W, cj):
    seen = set()
    for p in sr.aggregate_passes(W, cj):
        for r in (p["sel"][0], p["sel"][-1]):
            got = sr.reduce_strips(rasters[r], p["x0"], p["x1"], p["f"], p["strips"])
            assert got.dtype == np.uint8 and got.shape == (sum(p["cell_rows"]), p["Wa"])
            assert got.tolist() == cells_by_hand(rasters[r], p["x0"], p["x1"], p["f"], p["strips"]), (p["f"], r)
            seen |= set(got.ravel().tolist())
    return seen


@pytest.mark.parametrize("name", [k for k in sr.SPECS if k[0] == "E"])
def test_the_strip_wise_reduction_equals_a_loop_over_cells(tables, name):
    t = sr.host_tile(tables, name)
    passes = sr.aggregate_passes(t.W, t.cj)
    check_reduction({r: t.want(r) for p in passes for r in (p["sel"][0], p["sel"][-1])}, t.W, t.cj)


def test_the_strip_wise_reduction_equals_a_loop_over_cells_300_x_27():
    """Values of the whole byte range, a third of them 255, so that cells without a value and ties occur."""
    rng = np.random.default_rng(27)
    W, H = 300, 27
    raster = np.where(rng.integers(0, 3, size=(H, W)) == 0, 255, rng.integers(0, 256, size=(H, W))).astype(np.uint8)
    cj = np.minimum((np.arange(H) + 3) * 4 // (H + 3), 3).astype(np.int32)
    seen = check_reduction({r: raster for r in range(18)}, W, cj)
    assert 255 in seen and len(seen) > 100


def rasters_of(t, soil):
    return aggutil.oracle_rasters(t.esa, soil, t.tables)


def neighbour_soil(t):
    """The tile's soil with every column reading the soil cell next to its own."""
    return t.coarse[t.cj][:, (sr.clamp_columns(t.ci, t.hsx) + 1) % t.hsx]


def columns_that_differ(want, other):
    return np.any([(want[r] != other[r]).any(axis=0) for r in range(18)], axis=0)


def _sums(raster):
    v = raster.astype(np.int64)
    ok = v != 255
    return np.where(ok, v, 0), ok.astype(np.int64)


def _mean(s, n):
    out = np.full(s.shape, 255, np.int64)
    np.floor_divide(2 * s + n, 2 * n, out=out, where=n > 0)
    return out


def _over_cell_rows(a, strips, f):
    return np.vstack([np.add.reduceat(a[y0:y0 + rows], np.arange(0, rows, f), axis=0) for y0, rows in strips])


def columns_seen(p, want, other):
    """bool[W]: the columns x for which the bytes the pass expects change when column x ALONE is taken from `other`.
    Per cell s' = s - (the column's sum in the cell) + (the other column's), and likewise n: no reduction per column."""
    x0, x1, f = p["x0"], p["x1"], p["f"]
    W = want[p["sel"][0]].shape[1]
    starts, cell = np.arange(0, x1 - x0, f), np.arange(x1 - x0) // f
    seen = np.zeros(W, bool)
    for r in p["sel"]:
        col = [_over_cell_rows(a[:, x0:x1], p["strips"], f) for a in _sums(want[r]) + _sums(other[r])]
        s, n = (np.add.reduceat(a, starts, axis=1) for a in col[:2])
        swapped = _mean(s[:, cell] - col[0] + col[2], n[:, cell] - col[1] + col[3])
        seen[x0:x1] |= (swapped != _mean(s, n)[:, cell]).any(axis=0)
    return seen


def rows_unseen(t, p, want):
    """The rows y whose soil, replaced by the next soil row's, gives other full-resolution rasters in that row -- in
    the rasters and columns the pass reads -- and the same expected bytes.  Per cell as in columns_seen."""
    x0, x1, f = p["x0"], p["x1"], p["f"]
    other = rasters_of(t, t.coarse[(t.cj + 1) % t.hsy][:, sr.clamp_columns(t.ci, t.hsx)])
    differ = np.any([(want[r][:, x0:x1] != other[r][:, x0:x1]).any(axis=1) for r in p["sel"]], axis=0)
    starts = np.arange(0, x1 - x0, f)
    cell_row, first = np.zeros(t.H, np.int64), 0
    for (y0, rows), n in zip(p["strips"], p["cell_rows"]):
        cell_row[y0:y0 + rows] = first + np.arange(rows) // f
        first += n
    seen = np.zeros(t.H, bool)
    for r in p["sel"]:
        row = [np.add.reduceat(a[:, x0:x1], starts, axis=1) for a in _sums(want[r]) + _sums(other[r])]
        s, n = (_over_cell_rows(a, p["strips"], f) for a in row[:2])
        swapped = _mean(s[cell_row] - row[0] + row[2], n[cell_row] - row[1] + row[3])
        seen |= (swapped != _mean(s, n)[cell_row]).any(axis=1)
    return int(differ.sum()), np.flatnonzero(differ & ~seen).tolist()


# pass (b) BY ITSELF lets these columns through -- the only ones on any tile; pass (c), the same kernel, shows them
ONLY_PASS_C_SEES = {"E-5": [2], "E-17": [13]}


@pytest.mark.parametrize("name", [k for k, s in sr.SPECS.items() if s["hsx"] > 1])
def test_every_column_is_observable_by_both_aggregate_kernels(tables, name):
    """An area mean hides a wrong soil byte: a whole 40-row tile at f = 25 leaves up to 33 columns of these tiles
    (f = 16: up to 5) whose soil could be the neighbouring cell's without one expected byte changing.  The passes of
    the aggregate reader leave NONE, for either kernel, on any tile: every column whose full-resolution rasters differ
    anywhere between its soil and the neighbouring soil cell's changes, swapped alone, at least one expected byte of
    the pass for f < 16 and, separately, at least one of the passes for f >= 16."""
    t = sr.host_tile(tables, name)
    want, other = rasters_of(t, t.soil), rasters_of(t, neighbour_soil(t))
    for r in range(18):
        np.testing.assert_array_equal(want[r], t.want(r))
    counts = columns_that_differ(want, other)
    assert counts.sum() >= t.W // 2, "hardly a column of this tile would show its soil at full resolution"
    passes = sr.aggregate_passes(t.W, t.cj)
    seen = {p["f"]: columns_seen(p, want, other) for p in passes}
    assert not seen[25][:passes[2]["x0"]].any() and not seen[25][passes[2]["x1"]:].any()
    small, wide = seen[3], seen[16] | seen[25]
    assert passes[0]["form"] == sr.AGG_SMALL and passes[1]["form"] == passes[2]["form"] == sr.AGG_WIDE
    assert np.flatnonzero(counts & ~small).tolist() == [], sr.AGG_SMALL
    assert np.flatnonzero(counts & ~wide).tolist() == [], sr.AGG_WIDE
    assert np.flatnonzero(counts & ~seen[16]).tolist() == ONLY_PASS_C_SEES.get(name, []), "pass (b) alone"


@pytest.mark.parametrize("name,columns", [("E-5", range(5)), ("E-17", range(17)),
                                          ("A-zig-zag", (0, 1, 1039, 2046, 2047))])
def test_the_per_cell_update_equals_a_reduction_of_the_swapped_tile(tables, name, columns):
    """columns_seen against the statement it abbreviates: the oracle over the soil with ONE column swapped, reduced by
    the reader's own reference."""
    t = sr.host_tile(tables, name)
    want, soil2 = rasters_of(t, t.soil), neighbour_soil(t)
    other = rasters_of(t, soil2)
    passes = sr.aggregate_passes(t.W, t.cj)
    seen = [columns_seen(p, want, other) for p in passes]
    for x in columns:
        soil = t.soil.copy()
        soil[:, x] = soil2[:, x]
        swapped = rasters_of(t, soil)
        for p, s in zip(passes, seen):
            changed = any((sr.reduce_strips(swapped[r], p["x0"], p["x1"], p["f"], p["strips"]) !=
                           sr.reduce_strips(want[r], p["x0"], p["x1"], p["f"], p["strips"])).any() for r in p["sel"])
            assert changed == bool(s[x]), (x, p["f"])


@pytest.mark.parametrize("name", [k for k, s in sr.SPECS.items() if s["hsx"] == 1])
def test_one_soil_column_another_class_changes_bytes_of_both_kernels(tables, name):
    """hsx = 1: there is no neighbouring cell.  The whole tile on one other soil class, whichever of A to D, changes
    expected bytes of every pass."""
    t = sr.host_tile(tables, name)
    want = rasters_of(t, t.soil)
    judged = 0
    for hsg in (1, 2, 3, 4):
        other = rasters_of(t, np.full_like(t.soil, hsg))
        if not any((want[r] != other[r]).any() for r in range(18)):
            continue
        judged += 1
        for p in sr.aggregate_passes(t.W, t.cj):
            assert any((sr.reduce_strips(other[r], p["x0"], p["x1"], p["f"], p["strips"]) !=
                        sr.reduce_strips(want[r], p["x0"], p["x1"], p["f"], p["strips"])).any() for r in p["sel"]), \
                (hsg, p["f"])
    assert judged >= 3


@pytest.mark.parametrize("name", [k for k, s in sr.SPECS.items() if s["hsy"] > 1])
def test_every_soil_row_is_observable_by_the_row_walk(tables, name):
    """Pass (c) walks the rows of a cell row across changing soil rows: one strip row on the NEXT soil row's soil
    changes an expected byte wherever it changes the full-resolution rasters the pass reads in that row."""
    t = sr.host_tile(tables, name)
    p = sr.aggregate_passes(t.W, t.cj)[2]
    judged, unseen = rows_unseen(t, p, rasters_of(t, t.soil))
    assert unseen == []
    assert judged >= t.H // 2       # (a tile on ONE soil column, A-constant, has soil rows of the same class)


# ---- the reference of the grid reader --------------------------------------------------------------------------------

def words_by_hand(p, rasters):
    """The words of a pass in Python integers, strip by strip and cell by cell: {s, n, sum of every table's weight} over
    the values != 255 of the cell's pixels."""
    cellx, celly, ws = p["cellx"].tolist(), p["celly"].tolist(), [w.tolist() for w in p["ws"]]
    columns = [[x for x in range(len(cellx)) if cellx[x] == cx] for cx in range(p["ncx"])]
    out = []
    for r in p["sel"]:
        v = np.asarray(rasters[r]).tolist()
        acc = [[[0] * p["words"] for _cx in range(p["ncx"])] for _cy in range(p["ncy"])]
        for y0, rows in p["strips"]:
            for cy in range(p["ncy"]):
                ys = [y for y in range(y0, y0 + rows) if celly[y] == cy]
                for cx in range(p["ncx"] if ys else 0):
                    cell = acc[cy][cx]
                    for x in columns[cx]:
                        for y in ys:
                            value = v[y][x]
                            if value != 255:
                                cell[0] += value
                                cell[1] += 1
                                for j, w in enumerate(ws):
                                    cell[2 + j] += w[value]
        out.append(acc)
    return out


@pytest.mark.parametrize("name", [k for k in sr.SPECS if k[0] == "E"])
def test_the_strip_wise_sums_equal_a_loop_over_cells(tables, name):
    t = sr.host_tile(tables, name)
    for p in sr.grid_passes(t.W, t.H, t.cj)[1:] + [sr.weighted_rows_pass(t.W, t.H, t.cj)]:
        rasters = {r: t.want(r) for r in (p["sel"] if p["name"] == "storms" else p["sel"][:1])}
        p = dict(p, sel=list(rasters))
        got = sr.grid_words(p, rasters)
        assert got.dtype == np.int64 and got.shape == (len(rasters), p["ncy"], p["ncx"], p["words"])
        assert got.tolist() == words_by_hand(p, rasters), p["name"]
        assert (got[..., 2:].reshape(-1, len(p["ws"])).max(axis=0) > 0).all()      # every table weighs something here


def pixel_words(raster, ws):
    """int64[H][W][2 + k]: what every pixel adds to the words of its cell."""
    v = np.asarray(raster).astype(np.int64)
    ok = v != 255
    return np.stack([np.where(ok, v, 0), ok.astype(np.int64)] + [np.where(ok, w.astype(np.int64)[v], 0) for w in ws],
                    axis=-1)


def lines_seen(p, want, other, axis):
    """bool[W] (axis 1) or bool[H] (axis 0): the columns or rows whose pixels, taken from `other` ALONE, change a word
    the pass expects.  The words are sums over pixels, so per cell the change is the sum, over the line's pixels in that
    cell, of what each adds in `other` less what it adds in `want`; a strip only cuts these sums in two."""
    cellx, celly = p["cellx"].astype(np.int64), p["celly"].astype(np.int64)
    ys, xs = np.flatnonzero(celly >= 0), np.flatnonzero(cellx >= 0)
    seen = np.zeros(len(cellx) if axis else len(celly), bool)
    for r in p["sel"]:
        delta = pixel_words(other[r], p["ws"]) - pixel_words(want[r], p["ws"])
        if axis:            # a column: one change per cell row
            change = np.zeros((p["ncy"],) + delta.shape[1:], np.int64)
            np.add.at(change, celly[ys], delta[ys])
            seen[xs] |= (change != 0).any(axis=(0, 2))[xs]
        else:               # a row: one change per cell column
            change = np.zeros((p["ncx"], delta.shape[0], delta.shape[2]), np.int64)
            np.add.at(change, cellx[xs], delta[:, xs].transpose(1, 0, 2))
            seen[ys] |= (change != 0).any(axis=(0, 2))[ys]
    return seen


def other_soils(t):
    """(soil with every column on another class, soil with every row on another class): the neighbouring soil cell's
    and the next soil row's, or, where the window has one column or one row, each of the four classes in turn."""
    cols = [neighbour_soil(t)] if t.hsx > 1 else [np.full_like(t.soil, hsg) for hsg in (1, 2, 3, 4)]
    rows = [t.coarse[(t.cj + 1) % t.hsy][:, sr.clamp_columns(t.ci, t.hsx)]] if t.hsy > 1 else \
        [np.full_like(t.soil, hsg) for hsg in (1, 2, 3, 4)]
    return cols, rows


@pytest.mark.parametrize("name", list(sr.SPECS))
def test_every_soil_column_and_row_is_observable_by_the_grid_passes(tables, name):
    """The sums are exact, but a cell adds up many pixels.  One soil column on another class changes words of the `rows`
    pass wherever it changes a full-resolution raster, and one strip row on another soil row's soil changes words of
    the `storms` pass wherever it changes a raster the pass selects in a column it reads."""
    t = sr.host_tile(tables, name)
    want = rasters_of(t, t.soil)
    rows, storms = sr.grid_passes(t.W, t.H, t.cj)
    cols_soil, rows_soil = other_soils(t)
    judged = 0
    for soil in cols_soil:
        other = rasters_of(t, soil)
        differ = columns_that_differ(want, other)
        assert np.flatnonzero(differ & ~lines_seen(rows, want, other, 1)).tolist() == [], "rows pass"
        judged = max(judged, int(differ.sum()))
    assert judged >= t.W // 2, "hardly a column of this tile would show its soil at full resolution"
    judged = 0
    xs = storms["cellx"] >= 0
    for soil in rows_soil:
        other = rasters_of(t, soil)
        differ = np.any([(want[r][:, xs] != other[r][:, xs]).any(axis=1) for r in storms["sel"]], axis=0)
        differ &= storms["celly"] >= 0
        assert np.flatnonzero(differ & ~lines_seen(storms, want, other, 0)).tolist() == [], "storms pass"
        judged = max(judged, int(differ.sum()))
    assert judged >= (t.H - 5) // 2     # (a tile on ONE soil column, A-constant, has soil rows of the same class)


@pytest.mark.parametrize("name,columns,rows", [("E-5", range(5), range(3)), ("E-17", range(17), range(3)),
                                               ("A-zig-zag", (0, 4, 5, 1039, 2044, 2047), (0, 2, 3, 20, 37, 38))])
def test_the_per_line_change_equals_the_sums_of_the_swapped_tile(tables, name, columns, rows):
    """lines_seen against the statement it abbreviates: the oracle over the soil with ONE column or row swapped, summed
    by the reader's own reference."""
    t = sr.host_tile(tables, name)
    want = rasters_of(t, t.soil)
    cols_soil, rows_soil = other_soils(t)
    for axis, soil2, lines in ((1, cols_soil[0], columns), (0, rows_soil[0], rows)):
        other = rasters_of(t, soil2)
        passes = sr.grid_passes(t.W, t.H, t.cj)
        seen, words = [lines_seen(p, want, other, axis) for p in passes], [sr.grid_words(p, want) for p in passes]
        for i in lines:
            soil = t.soil.copy()
            if axis:
                soil[:, i] = soil2[:, i]
            else:
                soil[i] = soil2[i]
            swapped = rasters_of(t, soil)
            for p, s, w in zip(passes, seen, words):
                assert (sr.grid_words(p, swapped) != w).any() == bool(s[i]), (p["name"], axis, i)


def test_the_tiles_of_case_i_differ_in_more_than_half_of_their_soil():
    soils = sr.case_i_soils()
    for a, b in ((0, 1), (1, 2), (0, 2)):
        h, w = min(soils[a].shape[0], soils[b].shape[0]), min(soils[a].shape[1], soils[b].shape[1])
        assert (sr.soil_code(soils[a][:h, :w]) != sr.soil_code(soils[b][:h, :w])).mean() > 0.5, (a, b)
