"""The LZW model of tests/lzw_model.py and the crafted streams of tests/lzw_cases.py (CPU only): every family
reaches what it is there for (stated through the reference decoder's trace), the host reader (tiff_codec.c
lzw_decode) and libtiff read the streams as the model does, and every family tells the model from decoders
that are wrong in one of the classic ways.  The GPU decoder's tests rest on this."""
import collections
import contextlib

import numpy as np
import pytest
from PIL import Image

from gcn10_amd import host
from tests import lzw_cases as lc
from tests import tiffutil
from tests.lzw_model import (CLEAR, EOI, FIRST, MAXC, LzwCodeError, LzwError, LzwFirstError, LzwInputError,
                             LzwWriter, lzw_decode_ref, pack, width_of)

FAMILIES = list(lc.FAMILIES)


def _verdict(decode, case):
    try:
        return decode(case.stream, case.out_len)
    except LzwError as e:
        return type(e)


def _traces(cases):
    for c in cases:
        if isinstance(c.want, bytes):
            yield c, lzw_decode_ref(c.stream, c.out_len, trace=True)[1]


def test_old_names_still_import():
    from tests.test_gpu_lzw_input import pack as p2
    from tests.test_lzw_input_plan import lzw_decode_ref as ref2
    assert ref2 is lzw_decode_ref and p2 is pack
    assert issubclass(LzwCodeError, ValueError) and {e.status for e in (LzwCodeError, LzwFirstError, LzwInputError)} \
        == {9, 10, 11}


def test_writer_and_trace_agree_on_a_small_stream():
    w = LzwWriter()
    w.lit(65)
    w.lit(66)           # 258 = AB
    w.code(258)         # 259 = BA
    w.kwkwk()           # 260 = ABA, written as itself
    w.newest(1)         # 259
    w.eoi()
    assert w.codes == [CLEAR, 65, 66, 258, 260, 259, EOI] and bytes(w.out) == b"ABABABABA"
    data, tr = lzw_decode_ref(w.stream(), 8, trace=True)
    assert data == b"ABABABAB" and tr.end == "cap" and not tr.eois
    assert [(c.index, c.pos, c.length, c.literal, c.source, c.kwkwk, c.cut) for c in tr.codes] == [
        (0, 0, 1, 65, None, False, False), (1, 1, 1, 66, None, False, False), (2, 2, 2, None, 0, False, False),
        (3, 4, 3, None, 2, True, False), (4, 7, 2, None, 1, False, True)]
    assert [(m.index, m.width, m.bit) for m in tr.clears] == [(0, 9, 0)]
    data, tr = lzw_decode_ref(w.stream(), 12, trace=True)
    assert data == b"ABABABABA\0\0\0" and tr.end == "eoi" and [(m.index, m.bit, m.pos) for m in tr.eois] == [(5, 54, 9)]
    assert lzw_decode_ref(pack([FIRST]), 0) == b""              # an empty chunk reads no code
    assert [width_of(n) for n in (0, 253, 254, 765, 766, 1789, 1790, 5000)] == [9, 9, 10, 10, 11, 11, 12, 12]


@pytest.mark.parametrize("family", FAMILIES)
def test_model_decodes_every_case_to_what_its_writer_says(family):
    for c in lc.FAMILIES[family]():
        assert _verdict(lzw_decode_ref, c) == c.want, c.name


# ---- what every family is there for, through the trace -------------------------------------------------------

def _prop_clear_after_k(cases):
    at, widths, seen = set(), set(), collections.Counter()
    for c, tr in _traces(cases):
        seen["no_leading_clear"] += tr.clears[0].bit != 0
        for a, b in zip(tr.clears, tr.clears[1:]):
            seen["two_in_a_row"] += b.bit == a.bit + a.width
        for m in tr.clears:
            if m.bit:
                at.add(m.index)
                widths.add(m.width)
                seen["after_the_dictionary_filled"] += m.index > MAXC - FIRST
                assert tr.codes and any(k.pos >= m.pos for k in tr.codes)      # more data follows
    assert at >= set(lc.K) and widths == {9, 10, 11, 12}
    assert seen["no_leading_clear"] >= 50 and seen["two_in_a_row"] >= 1 and seen["after_the_dictionary_filled"] >= 5


def _prop_eoi_after_k(cases):
    at, seen = set(), collections.Counter()
    for c, tr in _traces(cases):
        assert tr.end == "eoi" and tr.eois[0].pos < c.out_len and not any(c.want[tr.eois[0].pos:])
        at.add(tr.eois[0].index)
        seen["first_code"] += tr.eois[0].bit == 0
        seen["right_after_a_clear"] += bool(tr.clears) and tr.clears[-1].bit + tr.clears[-1].width == tr.eois[0].bit
        seen["right_after_a_later_clear"] += (len(tr.clears) > 1
                                              and tr.clears[-1].bit + tr.clears[-1].width == tr.eois[0].bit)
    assert at >= set(lc.K)
    assert seen["first_code"] >= 2 and seen["right_after_a_clear"] >= 8 and seen["right_after_a_later_clear"] >= 7


def _prop_chunk_end(cases):
    at = collections.defaultdict(set)
    for c, tr in _traces(cases):
        how, last = c.tags[0], tr.codes[-1]
        assert tr.end == "cap" and len(tr.clears) == 1
        at[how].add(last.index)
        assert last.length >= min(3, last.index + 1)
        assert last.cut == (how != "exact")
        assert c.out_len == {"first": last.pos + 1, "last": last.pos + last.length - 1,
                             "exact": last.pos + last.length}[how]
        if not c.name.endswith("_none"):
            assert 8 * len(c.stream) - tr.bits_read >= 27          # codes follow, and are not read
            with pytest.raises(LzwError) if c.name.endswith("_invalid") else contextlib.nullcontext():
                lzw_decode_ref(c.stream, c.out_len + 600)           # (they are what their name says)
    assert at["exact"] == set(range(131)) and at["first"] == set(range(1, 131)) and at["last"] == set(range(2, 131))


def _prop_truncation(cases):
    cut = [c for c in cases if c.name.startswith("cut_to_")]
    assert [len(c.stream) for c in cut] == list(range(401)) and len({c.out_len for c in cut}) == 1
    ok = [c for c in cut if c.want is not LzwInputError]
    assert 40 <= len(ok) <= 100 and all(c.want is LzwInputError for c in cut if c not in ok)
    for c, tr in _traces(ok):
        assert tr.codes[-1].cut and tr.end == "cap"
    assert len({len(c.stream) % 4 for c in ok}) == 4
    # the refused lengths end inside a code far more often than between two
    whole = {(9 + sum(width_of(i) for i in range(n))) for n in range(700)}
    assert sum(1 for c in cut if 8 * len(c.stream) not in whole) > 300
    short = [c for c in cases if c.name.startswith("one_byte_short")]
    whole = [c for c in cases if c.name.startswith("whole_code")]
    assert len(short) == len(whole) == 140
    for i, (a, b) in enumerate(zip(whole, short)):
        # the chunk ends exactly in code i, whose last bits lie in the stream's last byte: the byte b lacks
        tr = lzw_decode_ref(a.stream, a.out_len, trace=True)[1]
        assert tr.end == "cap" and tr.codes[-1].index == i and not tr.codes[-1].cut
        assert 8 * (len(a.stream) - 1) < tr.bits_read <= 8 * len(a.stream)
        assert b.stream == a.stream[:-1] and b.out_len == a.out_len and b.want is LzwInputError


def _prop_invalid_code(cases):
    ks = set(range(1, 131)) | set(lc.NEAR_WIDTHS)
    by = collections.defaultdict(dict)
    for c in cases:
        kind, _, k = c.name.rpartition("_")
        if k.isdigit():
            by[kind][int(k)] = c
    assert set(by["next_plus_1_as_code"]) == set(by["next_as_code"]) == set(by["entry_after_clear_after"]) == ks
    for k in ks:
        bad, good, first = by["next_plus_1_as_code"][k], by["next_as_code"][k], by["entry_after_clear_after"][k]
        assert bad.want is LzwCodeError and first.want is LzwFirstError
        tr = lzw_decode_ref(good.stream, good.out_len, trace=True)[1]
        assert tr.codes[k].kwkwk and tr.codes[k].index == k and tr.codes[k].width == width_of(k)
        # the refused stream is the good one up to that code, whose value is one more
        _, tb = lzw_decode_ref(bad.stream, tr.codes[k].pos, trace=True)
        assert [x.code for x in tb.codes] == [x.code for x in tr.codes[:k]]
    # refused and good streams alternate
    kinds = [isinstance(c.want, bytes) for c in cases]
    assert all(kinds[i] or (kinds[i - 1] if i else True) or kinds[i + 1] for i in range(len(kinds) - 1))
    assert kinds[-1]


def _prop_kwkwk(cases):
    at, runs, after = set(), set(), []
    for c, tr in _traces(cases):
        run = 0
        for i, k in enumerate(tr.codes):
            run = run + 1 if k.kwkwk else 0
            if k.kwkwk:
                at.add(k.index)
                runs.add(run)
                s = c.want[k.pos:k.pos + k.length]
                assert s[-1] == s[0] and k.source == tr.codes[i - 1].pos and k.length == tr.codes[i - 1].length + 1
                if len(set(s)) > 2:
                    after.append(k.length - 1)
        if "kwkwk_as_code" in c.name and int(c.name.rsplit("_", 1)[1]) >= 3:
            k = tr.codes[int(c.name.rsplit("_", 1)[1])]
            s = c.want[k.pos:k.pos + k.length]
            assert k.kwkwk and s[-1] != s[-2]                       # a wrong wrap byte shows
    assert at >= set(range(1, 131)) and runs >= set(range(1, 71))
    assert sum(1 for n in after if n > 64) >= 4 and sum(1 for n in after if n > 200) >= 2


def _prop_source_distance(cases):
    seen = collections.defaultdict(set)
    for c, tr in _traces(cases):
        for k in tr.codes:
            if k.source is not None and not k.kwkwk and k.length in lc.ENTRY_LENGTHS:
                s = c.want[k.pos:k.pos + k.length]
                if len(set(s)) > 1 and c.want[k.source:k.source + k.length] == s:
                    seen[k.length].add(k.pos - k.source)
    for L in lc.ENTRY_LENGTHS:
        assert seen[L] >= {d for d in lc.DISTANCES if d >= L}, L


def _prop_dictionary_full(cases):
    seen = collections.Counter()
    for c, tr in _traces(cases):
        on_full = [k for k in tr.codes if k.index > MAXC - FIRST]
        assert len(on_full) >= 300 and all(k.width == 12 for k in on_full)
        assert {4093, 4094, 4095} <= {k.code for k in on_full}
        seen["kwkwk_makes_4095"] += any(k.kwkwk and k.code == MAXC - 1 for k in tr.codes)
        late = [m for m in tr.clears if m.width == 12]
        if late:
            after = [k for k in tr.codes if k.pos >= late[-1].pos]
            seen["clear_then_9_bits"] += len(after) >= 100 and after[0].width == 9
        seen["cut"] += tr.codes[-1].cut
    assert seen["kwkwk_makes_4095"] >= 3 and seen["clear_then_9_bits"] >= 4 and seen["cut"] == 2


def _prop_long_streams(cases):
    for c, tr in _traces(cases):
        assert len(c.stream) >= 4096 and len(tr.clears) >= 3
        gaps = {b.bit - a.bit for a, b in zip(tr.clears, tr.clears[1:])}
        assert len(gaps) >= 2 and len(gaps) >= len(tr.clears) // 4         # at irregular places
    assert max(len(c.stream) for c in cases) >= 16384
    assert {m.width for c, tr in _traces(cases) for m in tr.clears} == {9, 10, 11, 12}


@pytest.mark.parametrize("family", FAMILIES)
def test_family_reaches_what_it_is_there_for(family):
    globals()["_prop_" + family](lc.FAMILIES[family]())


def test_census_of_the_corpus(capsys):
    """The counts quoted at the head of tests/lzw_cases.py; every path the GPU decoder's older tests never
    or hardly reached is reached at least ten times."""
    cen = lc.census([c for f in FAMILIES for c in lc.FAMILIES[f]()])
    with capsys.disabled():
        print("\nLZW corpus: " + ", ".join("%s %d" % kv for kv in sorted(cen.items())))
    assert cen["cut_codes"] >= 250
    assert all(cen["clear_at_%d_bits" % w] >= 10 for w in (9, 10, 11, 12))
    assert cen["eoi_before_out_len"] >= 250 and cen["eoi_indices"] >= 250
    assert cen["end_indices"] >= 131 and cen["code_4095"] >= 10
    assert all(cen["refused_" + e.__name__] >= 100 for e in (LzwCodeError, LzwFirstError, LzwInputError))
    assert cen["max_distance"] > 4300


# ---- the host reader and libtiff ------------------------------------------------------------------------------

def _one_chunk_tiff(path, stream, out_len, monkeypatch):
    """A TIFF one pixel wide and out_len high whose single strip is the stream."""
    with monkeypatch.context() as m:
        m.setattr(tiffutil, "lzw_encode", lambda raw: bytes(stream))
        tiffutil.write_tiff(str(path), np.zeros((out_len, 1), np.uint8), compression=5)


@pytest.mark.parametrize("family", FAMILIES)
def test_host_reader_and_libtiff_read_every_case_as_the_model_does(family, tmp_path, monkeypatch):
    p = tmp_path / "c.tif"
    n_libtiff = 0
    for c in lc.FAMILIES[family]():
        if not c.stream:
            continue                    # a chunk of no bytes is a sparse chunk to the host reader: zeros
        _one_chunk_tiff(p, c.stream, c.out_len, monkeypatch)
        with host.Raster(str(p)) as r:
            if isinstance(c.want, bytes):
                assert r.read(0, 0, 1, c.out_len).tobytes() == c.want, c.name
            else:
                with pytest.raises(host.HostError):
                    r.read(0, 0, 1, c.out_len)
        if c.wellformed:
            with Image.open(str(p)) as im:
                assert im.tag_v2[259] == 5
                assert np.array(im).tobytes() == c.want, c.name
            n_libtiff += 1
    assert n_libtiff >= {"clear_after_k": 150, "invalid_code": 150, "kwkwk": 200, "source_distance": 1000,
                         "long_streams": 5}.get(family, 0)


# ---- decoders that are wrong in one way each ------------------------------------------------------------------

VARIANTS = ("late_width_change", "clear_keeps_the_width", "kwkwk_repeats_the_last_byte", "dictionary_stops_at_4095",
            "dictionary_grows_past_4096", "cut_code_dropped_whole", "eoi_ignored", "partial_last_code_zero_padded")

MUST_CATCH = {
    "clear_after_k": ("late_width_change", "clear_keeps_the_width", "dictionary_grows_past_4096"),
    "eoi_after_k": ("eoi_ignored", "late_width_change", "dictionary_grows_past_4096"),
    "chunk_end": ("cut_code_dropped_whole", "kwkwk_repeats_the_last_byte"),
    "truncation": ("partial_last_code_zero_padded", "cut_code_dropped_whole", "late_width_change"),
    "invalid_code": ("kwkwk_repeats_the_last_byte", "late_width_change"),
    "kwkwk": ("kwkwk_repeats_the_last_byte",),
    "source_distance": ("late_width_change",),
    "dictionary_full": ("dictionary_stops_at_4095", "dictionary_grows_past_4096", "clear_keeps_the_width",
                        "late_width_change"),
    "long_streams": ("late_width_change", "clear_keeps_the_width"),
}


def _wrong_decoder(v):
    """lzw_decode_ref with one mistake."""
    assert v in VARIANTS
    limit = {"dictionary_stops_at_4095": MAXC - 1, "dictionary_grows_past_4096": 1 << 30}.get(v, MAXC)
    max_width = 16 if v == "dictionary_grows_past_4096" else 12
    early = 0 if v == "late_width_change" else 1

    def decode(src, cap):
        out = bytearray()
        table = [bytes([i]) for i in range(256)] + [b"", b""]
        width, prev = 9, None
        bits = nbits = ip = 0
        padded = False
        if cap == 0:
            return b""
        while True:
            while nbits < width:
                if ip >= len(src):
                    if v == "partial_last_code_zero_padded" and nbits and not padded:
                        bits, nbits, padded = bits << 8, nbits + 8, True
                        continue
                    if len(out) >= cap:
                        return bytes(out[:cap])
                    raise LzwInputError()
                bits = (bits << 8) | src[ip]
                ip += 1
                nbits += 8
            code = (bits >> (nbits - width)) & ((1 << width) - 1)
            nbits -= width
            if code == EOI:
                if v == "eoi_ignored":
                    continue
                return bytes(out[:cap]) + bytes(max(0, cap - len(out)))
            if code == CLEAR:
                del table[FIRST:]
                prev = None
                if v != "clear_keeps_the_width":
                    width = 9
                continue
            if prev is None:
                if code >= 256:
                    raise LzwFirstError()
                s = table[code]
            else:
                nxt = len(table)
                if code > nxt or (code == nxt and nxt >= limit):
                    raise LzwCodeError()
                if code == nxt:
                    s = table[prev] + (table[prev][-1:] if v == "kwkwk_repeats_the_last_byte" else table[prev][:1])
                else:
                    s = table[code]
                if nxt < limit:
                    table.append(table[prev] + s[:1])
                if len(table) + early >= (1 << width) and width < max_width:
                    width += 1
            if v == "cut_code_dropped_whole" and len(out) + len(s) > cap:
                return bytes(out) + bytes(cap - len(out))
            out += s
            prev = code
            if len(out) >= cap:
                return bytes(out[:cap])
    return decode


def test_every_variant_has_a_family_that_must_catch_it():
    assert set(MUST_CATCH) == set(FAMILIES)
    assert {v for vs in MUST_CATCH.values() for v in vs} == set(VARIANTS)


@pytest.mark.parametrize("family,variant", [(f, v) for f in FAMILIES for v in MUST_CATCH[f]])
def test_family_tells_the_model_from_a_wrong_decoder(family, variant):
    wrong = _wrong_decoder(variant)
    caught = sum(1 for c in lc.FAMILIES[family]() if _verdict(wrong, c) != c.want)
    assert caught >= 1, (family, variant)
