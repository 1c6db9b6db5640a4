"""CPU: the references of tests/test_gpu_soil_readers.py checked against an independent statement of each -- the
column rule value by value, plain indexing against the oracle's resample loop, the per-zone counts against the pair
histogram of the whole strip -- and the shapes the reader tests rely on."""
import numpy as np
import pytest

from gcn10_amd import host
from oracle import cn_oracle_c as oc
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


def test_the_tiles_of_case_i_differ_in_more_than_half_of_their_soil():
    soils = sr.case_i_soils()
    for a, b in ((0, 1), (1, 2), (0, 2)):
        h, w = min(soils[a].shape[0], soils[b].shape[0]), min(soils[a].shape[1], soils[b].shape[1])
        assert (sr.soil_code(soils[a][:h, :w]) != sr.soil_code(soils[b][:h, :w])).mean() > 0.5, (a, b)
