"""The zlib stream model of tests/deflate_model.py against zlib itself (CPU only): it must decode what zlib and
libdeflate write exactly as zlib does, and accept or refuse every hand-made stream of tests/deflate_cases.py
exactly as zlib does, with zlib's reason.  The GPU decoder and encoder tests rest on it."""
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

from tests import deflate_cases as dc
from tests import deflate_model as dm
from tests.conftest import GOLDEN

CORPUS = os.path.join(GOLDEN, "deflate")


def _corpus():
    with open(os.path.join(CORPUS, "manifest.json")) as f:
        man = json.load(f)
    for e in man:
        with open(os.path.join(CORPUS, e["file"]), "rb") as f:
            yield e, f.read()


def _data(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "classes":
        runs = rng.geometric(0.05, size=n // 8 + 16)
        return np.repeat(rng.integers(0, 11, len(runs)).astype(np.uint8) * 10, runs)[:n].tobytes()
    if kind == "noise":
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "skewed":
        return np.minimum(rng.geometric(0.35, n), 255).astype(np.uint8).tobytes()
    if kind == "period":
        return np.tile(rng.integers(0, 256, 37, dtype=np.uint8), n // 37 + 1)[:n].tobytes()
    raise ValueError(kind)


def _same_as_zlib(stream):
    got, reason = dm.zlib_verdict(stream)
    mine, my_reason = dm.model_verdict(stream)
    assert (mine, my_reason) == (got, reason)
    return got


@pytest.mark.parametrize("kind", ["classes", "noise", "skewed", "period"])
@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_reader_equals_zlib_on_zlib_streams(kind, level):
    raw = _data(kind, 70000, level)
    for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_RLE, zlib.Z_HUFFMAN_ONLY):
        c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
        st = c.compress(raw[:30000]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(raw[30000:]) + c.flush()
        r = dm.read(st)
        assert r.data == raw and r.end == len(st) and r.adler_ok
        assert all(b.type in (0, 1, 2) for b in r.blocks) and r.blocks[-1].final
        assert r.blocks[-1].end_bit <= 8 * (len(st) - 4)
        # the tokens are the bytes
        out = bytearray()
        for b in r.blocks:
            if b.type == 0:
                continue
            for t in b.tokens:
                if t[0] == "lit":
                    out.append(t[1])
                elif t[0] == "match":
                    for _ in range(t[1]):
                        out.append(out[-t[2]])
        assert len(out) <= len(raw)


def test_reader_reports_where_the_stream_ends_and_a_wrong_checksum():
    raw = _data("classes", 5000, 1)
    st = zlib.compress(raw, 6)
    r = dm.read(st + b"trailing bytes")             # zlib stops at the end of the stream, and so does the model
    assert r.data == raw and r.end == len(st)
    assert _same_as_zlib(st + b"xyz") == raw
    bad = st[:-4] + ((int.from_bytes(st[-4:], "big") + 1) & 0xFFFFFFFF).to_bytes(4, "big")
    assert dm.zlib_verdict(bad) == (None, "incorrect data check") == dm.model_verdict(bad)
    r = dm.read(bad, check_adler=False)
    assert r.data == raw and not r.adler_ok
    for cut in (1, 2, 5, len(st) // 2, len(st) - 4, len(st) - 1):
        assert dm.model_verdict(st[:cut]) == (None, dm.TRUNCATED) == dm.zlib_verdict(st[:cut])


def test_reader_equals_zlib_on_corrupted_streams():
    rng = np.random.default_rng(3)
    raw = _data("classes", 20000, 2) + _data("skewed", 20000, 3)
    good = [zlib.compress(raw, lvl) for lvl in (1, 6, 9)]
    refused = 0
    for k in range(300):
        b = bytearray(good[k % 3])
        for _ in range(1 + k % 3):
            b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))
        refused += _same_as_zlib(bytes(b)) is None
    assert refused > 250


def test_reader_equals_zlib_on_the_libdeflate_corpus():
    n = 0
    for e, st in _corpus():
        r = dm.read(st)
        assert hashlib.sha256(r.data).hexdigest() == e["sha256"] and len(r.data) == e["size"], e["file"]
        assert r.end == len(st) and r.adler_ok
        assert zlib.decompress(st) == r.data
        n += 1
    levels = {e["level"] for e, _ in _corpus()}
    assert n >= 28 and levels == {1, 6, 9, 12}
    assert sum(os.path.getsize(os.path.join(CORPUS, e["file"])) for e, _ in _corpus()) < 600 * 1024


def test_corpus_holds_the_forms_it_is_there_for():
    """libdeflate's streams use forms zlib's encoder never writes: length-3 matches more than 4096 back (zlib
    levels 4-9 drop them), level 12's near-optimal parse."""
    far3 = {}
    for e, st in _corpus():
        r = dm.read(st)
        far3[e["file"]] = sum(1 for b in r.blocks for t in b.tokens if t[0] == "match" and t[1] == 3 and t[2] > 4096)
    assert sum(far3.values()) > 1000
    assert far3["words_64x256_L12.zz"] > 100


def test_reader_equals_libdeflate_where_it_is_installed():
    """Fresh libdeflate streams of levels 1 / 6 / 9 / 12 (where the library loads: the corpus above covers the
    machines where it does not)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_deflate_corpus", os.path.join(GOLDEN, "make_deflate_corpus.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    lib = mk.load_libdeflate()
    raws = [_data("classes", 40000, 7), _data("skewed", 30000, 8), mk.texture("words", 32, 256, 5).tobytes()]
    for raw in raws:
        for level in (1, 6, 9, 12):
            st = mk.compress(lib, raw, level) if lib is not None else zlib.compress(raw, min(level, 9))
            r = dm.read(st)
            assert r.data == raw and r.end == len(st) and r.adler_ok
            if lib is not None:
                assert mk.decompress_exact(lib, st, len(raw)) == raw


@pytest.mark.parametrize("case", dc.valid_cases(), ids=lambda c: c[0])
def test_crafted_valid_streams_decode_as_zlib_decodes_them(case):
    name, st, raw = case
    assert _same_as_zlib(st) == raw
    r = dm.read(st)
    assert r.end == len(st)
    dyn = [b for b in r.blocks if b.type == 2]
    if name.startswith("crossing_"):
        assert dyn[0].crossing
        sym = int(name[-2:])
        hl = dyn[0].hlit
        have, crossing_syms = 0, set()
        for s, ex in dyn[0].cl_items:
            rep = 1 if s < 16 else (3 + ex if s < 18 else 11 + ex)
            if have < hl < have + rep:
                crossing_syms.add(s)
            have += rep
        assert sym in crossing_syms
    if name == "fifteen_bit_codes_hclen19":
        assert dyn[0].hclen == 19 and max(dyn[0].lit_lens) == 15 and max(dyn[0].dist_lens) == 15
    if name.startswith("hlit257"):
        assert dyn[0].hlit == 257 and not any(dyn[0].dist_lens)
    if name.startswith("hlit286"):
        assert dyn[0].hlit == 286 and sum(1 for L in dyn[0].dist_lens if L) == 1
    if name == "hclen5":
        assert dyn[0].hclen == 5
    if name == "only_end_of_block_and_empty_blocks":
        assert [b.type for b in r.blocks] == [2, 1, 0, 1, 2, 0]
        assert dyn[0].tokens == [("eob",)] and sum(1 for L in dyn[0].lit_lens if L) == 1
    if name.startswith("length_258"):
        m = [t for t in dyn[0].tokens if t[0] == "match"]
        assert (258, 1, 284, 0) == m[0][1:] and (258, 1, 285, 0) == m[1][1:]
        assert sum(1 for t in m if t[1] == 3 and t[2] > 4096) == 60
    if name.startswith("distance_32768"):
        assert [b.type for b in r.blocks] == [0, 1, 0, 2] and r.blocks[0].stored_len == 65535
        assert sum(1 for b in r.blocks for t in b.tokens if t[0] == "match" and t[2] == 32768) == 6


def test_crafted_end_of_block_lands_on_every_bit_offset():
    offs = set()
    for name, st, raw in dc.valid_cases():
        if name.startswith("end_of_block_after_"):
            r = dm.read(st)
            offs.add((r.blocks[0].end_bit - 7) % 32)        # the first block's end of block (7 bits) starts here
            offs.add((r.blocks[1].end_bit - 7) % 32)
    assert offs == set(range(32))


@pytest.mark.parametrize("case", dc.invalid_cases(), ids=lambda c: c[0])
def test_crafted_invalid_streams_are_refused_as_zlib_refuses_them(case):
    name, st, reason, _ = case
    assert dm.zlib_verdict(st) == (None, reason)
    assert dm.model_verdict(st) == (None, reason)


def test_huffman_helpers():
    rng = np.random.default_rng(4)
    fib = [1, 1]
    while len(fib) < 25:
        fib.append(fib[-1] + fib[-2])
    assert max(dm.huffman_depths(fib)) == 24
    for freqs in (fib, list(rng.integers(0, 1000, 286)), [5], [0, 3, 0, 9]):
        for limit in (7, 15):
            if sum(1 for f in freqs if f) > 1 << limit:
                continue
            L = dm.limited_lengths(freqs, limit)
            assert max(L) <= limit and all((L[i] > 0) == (freqs[i] > 0) for i in range(len(freqs)))
            kraft = sum(2.0 ** -x for x in L if x)
            assert kraft == 1.0 or (kraft == 0.5 and sum(1 for x in L if x) == 1)
