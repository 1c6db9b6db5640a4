"""Hand-made TIFF LZW code streams for the GPU LZW decoder (gcn10_lzw_decode.hip) and the host reader,
written code by code with tests/lzw_model.LzwWriter.

FAMILIES maps a family's name to a function that returns its cases: Case(name, stream, out_len, want,
wellformed, tags).  want is the chunk's bytes (from the writer's own dictionary, not from the reference decoder)
or the LzwError the stream must end in.  wellformed: the stream starts with a Clear, ends with EOI, decodes to
exactly out_len bytes and never runs on a full table, so libtiff must read it alike.  What a family is there for
is stated through the reference decoder's trace (the PROPERTIES checked by tests/test_lzw_model.py), never
through a constant of the kernel: every sweep has at least 130 consecutive values, so that every alignment to
a batch of 64 codes or a step of 64 bytes occurs whatever those constants become.

What the corpus reaches, counted from the traces (census(); tests/test_lzw_model.py prints and checks it):
    streams 4429, decoded bytes 13.9 M, data codes 0.81 M
    cut codes (the last code straddles out_len): 1093
    Clears read at 9 / 10 / 11 / 12 bits: 3879 / 25 / 24 / 30
    EOIs read before out_len: 261, after 252 different numbers of codes
    chunks that end in the j-th code since the Clear: 363 different j, every one of 0..130 among them
    refusals: code beyond the dictionary 151, first code not a literal 152, input ended 486
    codes naming entry 4095: 383; KwKwK codes: 49409
    largest source distance: 24454 bytes
"""
import collections
import functools
import random

from tests.lzw_model import (CLEAR, EOI, FIRST, MAXC, LzwCodeError, LzwError, LzwFirstError, LzwInputError, LzwWriter,
                             lzw_decode_ref, pack, width_of)

Case = collections.namedtuple("Case", "name stream out_len want wellformed tags")

# every k in 0..199, and +-6 around the width changes (codes 254 / 766 / 1790 after a Clear) and the last
# code that makes an entry (3838)
K = sorted(set(range(200)) | {c + d for c in (254, 766, 1790, 3838) for d in range(-6, 7)})
NEAR_WIDTHS = sorted({c + d for c in (254, 766, 1790) for d in range(-3, 4)})


def grow(w, k, rng, literals=0.5):
    """k more codes: literals, KwKwK and live entries (the newest three more often than their share)."""
    for _ in range(k):
        r = rng.random()
        if w.prev is None or w.next == FIRST or r < literals:
            w.lit(rng.randrange(256))
        elif r < literals + 0.1 and not w.full:
            w.kwkwk()
        elif r < literals + 0.25:
            w.code(max(FIRST, w.next - 1 - rng.randrange(3)))
        else:
            w.code(rng.randrange(FIRST, w.next))


def chain(w, s):
    """Makes entries whose strings are s[:2], s[:3] ... s[:len(s)] (two codes each); returns {length: entry}."""
    w.lit(s[0])
    made = {2: w.next}
    w.lit(s[1])
    for k in range(2, len(s)):
        w.code(made[k])
        made[k + 1] = w.next
        w.lit(s[k])
        assert w.string(made[k + 1]) == bytes(s[:k + 1])
    return made


def _case(name, stream, out_len, want, tags=()):
    wf = False
    if isinstance(want, (bytes, bytearray)):
        want = bytes(want[:out_len]) + bytes(max(0, out_len - len(want)))
        if "maybe-wellformed" in tags:
            try:
                _, tr = lzw_decode_ref(stream, out_len + 1, trace=True)     # one more byte: reads on to the EOI
                wf = (bool(tr.clears) and tr.clears[0].bit == 0 and tr.end == "eoi" and tr.eois[0].pos == out_len
                      and all(c.index <= MAXC - FIRST for c in tr.codes))
            except LzwError:
                pass
    return Case(name, bytes(stream), out_len, want, wf, tuple(t for t in tags if t != "maybe-wellformed"))


def _finish(name, w, out_len=None, tags=()):
    """EOI, and the writer's bytes as the expectation."""
    w.eoi()
    return _case(name, w.stream(), len(w.out) if out_len is None else out_len, w.out, ("maybe-wellformed",) + tuple(tags))


@functools.lru_cache(None)
def clear_after_k():
    """A Clear after k codes, then 70 more codes.  k = 0: two Clears in a row (or a stream that starts with
    one where it need not).  Every third stream does not start with a Clear.  Beyond 3838 the Clear comes after
    the dictionary has filled."""
    rng, cases = random.Random(101), []
    for k in K + [3900, 4500]:
        w = LzwWriter(clear=k % 3 != 1)
        grow(w, k, rng)
        w.clear()
        grow(w, 70, rng)
        cases.append(_finish("clear_after_%d" % k, w))
    return cases


@functools.lru_cache(None)
def eoi_after_k():
    """EOI after k codes with out_len larger: zeros follow.  EOI as the first code, right after the leading
    Clear (k = 0), and right after a Clear in mid-stream."""
    rng, cases = random.Random(102), []
    for k in K:
        w = LzwWriter()
        grow(w, k, rng)
        cases.append(_finish("eoi_after_%d" % k, w, len(w.out) + 1 + (k * 7) % 150))
    cases.append(_case("eoi_first", pack([EOI]), 77, b""))
    cases.append(_case("eoi_only_after_garbage_free_start", pack([EOI, 65, 66]), 1, b""))
    for k in (1, 63, 64, 65, 127, 128, 300):
        w = LzwWriter()
        grow(w, k, rng)
        w.clear()
        cases.append(_finish("eoi_after_clear_after_%d" % k, w, len(w.out) + 200))
    return cases


def _last_code(w, j, rng):
    """Codes 0 .. j since the Clear, the j-th as long as a j-th code can be: a literal (j = 0), a KwKwK of
    two bytes (j = 1), "aaa" (j = 2), and from j = 3 on the KwKwK "aba", whose last byte is not its second."""
    if j == 0:
        return w.lit(97)
    if j == 1:
        w.lit(97)
        return w.kwkwk()
    if j == 2:
        w.lit(97)
        w.kwkwk()
        return w.kwkwk()
    grow(w, j - 3, rng)
    a, b = rng.sample(range(256), 2)
    w.lit(a)
    ab = w.next
    w.lit(b)
    w.code(ab)
    return w.kwkwk()


@functools.lru_cache(None)
def chunk_end():
    """The chunk ends in the j-th code since the Clear, j = 0..130: cut after the code's first byte, cut before
    its last byte, or exactly at its end; then nothing, valid codes, invalid codes or a Clear follow, all of
    them padding."""
    rng, cases = random.Random(103), []
    for j in range(131):
        w = LzwWriter()
        length = _last_code(w, j, rng)
        L = len(w.out)
        assert w.n == j + 1
        big = (1 << width_of(w.n)) - 1                       # > next at this width
        trailers = {"none": [], "valid": [w.codes[-2] if j else 98, 99, EOI], "invalid": [big, big, 300],
                    "clear": [CLEAR, 1, 2, 3, EOI]}
        for how, out_len in (("first", L - length + 1), ("last", L - 1), ("exact", L)):
            if (how == "first" and length < 2) or (how == "last" and length < 3):
                continue
            for tname, t in trailers.items():
                cases.append(_case("end_in_code_%d_%s_then_%s" % (j, how, tname), pack(w.codes + t), out_len,
                                   w.out, ("maybe-wellformed", how)))
    return cases


@functools.lru_cache(None)
def truncation():
    """One stream of 640 codes whose chunk ends inside the 300th: cut at every byte length 0..400 (the chunk's
    last code ends in byte 340 or so, so both verdicts occur, and most lengths leave part of a code).  And the
    chunk ending exactly in code i, i = 0..139, the stream ending with that code's last bits -- and one byte
    short of that: a decoder that reads the missing bits as zeros completes the chunk."""
    rng, cases = random.Random(104), []
    w = LzwWriter()
    _last_code(w, 300, rng)                                 # 3 bytes long
    out_len = len(w.out) - 1
    n_used = w.n
    grow(w, 640 - w.n, rng)
    w.eoi()
    s = w.stream()
    assert len(s) > 600
    bits = sum(width_of(i) for i in range(n_used)) + 9      # the leading Clear
    for n in range(401):
        enough = 8 * n >= bits
        cases.append(_case("cut_to_%d_bytes" % n, s[:n], out_len, w.out if enough else LzwInputError,
                           ("ok",) if enough else ()))
    w = LzwWriter()
    bit = 9
    for i in range(140):
        grow(w, 1, rng)
        bit += width_of(i)
        cases.append(_case("whole_code_%d" % i, w.stream()[:(bit + 7) // 8], len(w.out), w.out))
        cases.append(_case("one_byte_short_of_code_%d" % i, w.stream()[:(bit - 1) // 8], len(w.out), LzwInputError))
    return cases


@functools.lru_cache(None)
def invalid_code():
    """As the k-th code: next + 1 (refused), next itself (a valid KwKwK), and a non-literal right after a Clear
    placed there (refused).  k = 1..130 and around each width change.  Refused and good streams alternate, so a
    refused tile has good neighbours."""
    rng, cases = random.Random(105), []
    for k in list(range(1, 131)) + NEAR_WIDTHS:
        state = rng.getstate()
        w = LzwWriter()
        grow(w, k, rng)
        w.raw(w.next + 1)
        w.raw(65)
        w.eoi()
        cases.append(_case("next_plus_1_as_code_%d" % k, w.stream(), len(w.out) + 50, LzwCodeError))
        rng.setstate(state)
        w = LzwWriter()
        grow(w, k, rng)
        w.kwkwk()
        cases.append(_finish("next_as_code_%d" % k, w))
        w = LzwWriter()
        grow(w, k, rng)
        w.clear()
        w.raw(FIRST + rng.randrange(min(k, 250)))
        w.eoi()
        cases.append(_case("entry_after_clear_after_%d" % k, w.stream(), len(w.out) + 50, LzwFirstError))
    cases.append(_case("entry_as_first_code", pack([FIRST, EOI]), 10, LzwFirstError))
    cases.append(_case("good_last", pack([CLEAR, 1, 2, 3, EOI]), 3, b"\1\2\3", ("maybe-wellformed",)))
    return cases


@functools.lru_cache(None)
def kwkwk():
    """KwKwK as the k-th code, k = 1..130, after a string whose first and last bytes differ (from k = 3 on);
    runs of 1..70 KwKwK codes in a row; KwKwK after strings of 65, 70, 201 and 260 bytes of noise."""
    rng, cases = random.Random(106), []
    for k in range(1, 131):
        w = LzwWriter()
        if k < 3:
            grow(w, k, rng, literals=1.0)
            w.kwkwk()
        else:
            _last_code(w, k, rng)
        grow(w, 5, rng)
        cases.append(_finish("kwkwk_as_code_%d" % k, w))
    for run in range(1, 71):
        w = LzwWriter()
        grow(w, run % 7, rng)
        a, b = rng.sample(range(256), 2)
        w.lit(a)
        ab = w.next
        w.lit(b)
        w.code(ab)
        for _ in range(run):
            w.kwkwk()
        grow(w, 3, rng)
        cases.append(_finish("kwkwk_run_of_%d" % run, w))
    for L in (65, 70, 201, 260):
        w = LzwWriter()
        s = bytes(rng.randrange(256) for _ in range(L))
        made = chain(w, s)
        w.code(made[L])
        w.kwkwk()
        w.kwkwk()
        grow(w, 3, rng)
        cases.append(_finish("kwkwk_after_%d_bytes" % L, w, tags=("long",)))
    return cases


ENTRY_LENGTHS = (2, 3, 63, 64, 65, 200)
DISTANCES = list(range(1, 201)) + list(range(3900, 4301))


def _advance(w, made, gap):
    """gap more bytes of output from the chain's entries (and a literal where one byte is left)."""
    top = max(made)
    while gap:
        step = min(gap, top)
        if step == 1:
            w.lit(w.out[-1] ^ 0x55)
        else:
            w.code(made[step])
        gap -= step


@functools.lru_cache(None)
def source_distance():
    """A code that names an older entry of 2, 3, 63, 64, 65 or 200 bytes of noise whose string first lay d
    bytes back, d = 1..200 and 3900..4300 (a string that is not KwKwK lies at least its own length back, so
    an entry of L bytes has d >= L)."""
    cases = []
    for d in DISTANCES:
        rng = random.Random(107000 + d)
        for top in ((65, 200) if d >= 200 else (65,)):
            if top == 65 and d < 2:
                continue
            s = bytearray(rng.randrange(256) for _ in range(top))
            s[1] ^= s[1] == s[0]                            # (no entry is constant)
            w = LzwWriter()
            want = [L for L in ENTRY_LENGTHS if L <= min(d, top) and (top == 65 or L == 200)]
            if d <= 200:
                # inside the chain: the step that reads s[:L] back is delayed by d - L literals
                w.lit(s[0])
                made = {2: w.next}
                w.lit(s[1])
                for k in range(2, top + 1):
                    if k in want:
                        for _ in range(d - k):
                            w.lit(rng.randrange(256))
                        assert len(w.out) - w.source(made[k]) == d
                    if k == top and k not in want:
                        break
                    w.code(made[k])
                    if k < top:
                        made[k + 1] = w.next
                        w.lit(s[k])
            else:
                made = chain(w, s)
                for L in want:
                    _advance(w, made, w.source(made[L]) + d - len(w.out))
                    assert len(w.out) - w.source(made[L]) == d
                    w.code(made[L])
            grow(w, 2, rng)
            cases.append(_finish("entries_up_to_%d_at_distance_%d" % (top, d), w,
                                 tags=tuple("L%d" % L for L in want) + ("d%d" % d,)))
    return cases


@functools.lru_cache(None)
def dictionary_full():
    """More than 3838 codes without a Clear; a KwKwK that makes entry 4095; codes 4093, 4094, 4095; hundreds
    of 12-bit codes on the full dictionary; then a Clear and 9-bit codes again."""
    cases = []
    for seed, literals, kw_last, cut in ((1, 0.5, True, 0), (2, 0.9, True, 0), (3, 0.3, False, 0), (4, 0.5, True, 2),
                                         (5, 1.0, True, 0), (6, 0.5, False, 1)):
        rng = random.Random(108000 + seed)
        w = LzwWriter(clear=seed % 2 == 1)
        grow(w, MAXC - FIRST, rng, literals)
        assert w.next == MAXC - 1
        if kw_last:
            w.kwkwk()
        else:
            grow(w, 1, rng, literals)
        assert w.full
        for c in (4093, 4094, 4095, 4095, 4094):
            w.code(c)
        for i in range(600):
            w.code(rng.choice((rng.randrange(256), rng.randrange(FIRST, MAXC), MAXC - 1 - rng.randrange(4))))
        if cut:
            while len(w.out) - w.starts[-1] < 3:
                w.code(rng.randrange(FIRST, MAXC))
            cases.append(_case("full_%d_cut" % seed, pack(w.codes + [0xFFF, CLEAR, 5]), len(w.out) - cut, w.out))
            continue
        w.clear()
        grow(w, 100, rng)
        cases.append(_finish("full_%d" % seed, w, tags=("kw4095",) if kw_last else ()))
    return cases


@functools.lru_cache(None)
def long_streams():
    """At least 4 KiB of input each (one of 16 KiB), Clears at irregular places."""
    cases = []
    for seed, literals, lo, hi, size in ((1, 1.0, 30, 900, 4200), (2, 0.5, 30, 900, 4200), (3, 0.7, 1, 60, 4200),
                                         (4, 0.5, 2000, 4200, 6000), (5, 0.4, 300, 2500, 16500),
                                         (6, 0.05, 100, 1500, 4200)):
        rng = random.Random(109000 + seed)
        w = LzwWriter()
        bits = 9
        while bits < 8 * size:
            for _ in range(rng.randrange(lo, hi)):
                bits += width_of(w.n)
                grow(w, 1, rng, literals)
            bits += width_of(w.n)
            w.clear()
        grow(w, 5, rng, literals)
        cases.append(_finish("long_%d" % seed, w))
        assert len(cases[-1].stream) >= size
    return cases


FAMILIES = collections.OrderedDict([
    ("clear_after_k", clear_after_k), ("eoi_after_k", eoi_after_k), ("chunk_end", chunk_end),
    ("truncation", truncation), ("invalid_code", invalid_code), ("kwkwk", kwkwk),
    ("source_distance", source_distance), ("dictionary_full", dictionary_full), ("long_streams", long_streams)])


def census(cases):
    """What a set of cases reaches, from the reference decoder's traces."""
    c = collections.Counter()
    eoi_at, end_at = set(), set()
    for case in cases:
        c["streams"] += 1
        try:
            data, tr = lzw_decode_ref(case.stream, case.out_len, trace=True)
        except (LzwCodeError, LzwFirstError, LzwInputError) as e:
            c["refused_" + type(e).__name__] += 1
            continue
        c["bytes"] += len(data)
        c["codes"] += len(tr.codes)
        for m in tr.clears:
            c["clear_at_%d_bits" % m.width] += 1
        for m in tr.eois:
            if m.pos < case.out_len:
                c["eoi_before_out_len"] += 1
                eoi_at.add(m.index)
        if tr.end == "cap" and tr.codes:
            end_at.add(tr.codes[-1].index)
            c["cut_codes"] += tr.codes[-1].cut
        for k in tr.codes:
            c["kwkwk"] += k.kwkwk
            if k.source is not None:
                c["max_distance"] = max(c["max_distance"], k.pos - k.source)
        c["code_4095"] += sum(1 for k in tr.codes if k.code == MAXC - 1)
    c["eoi_indices"] = len(eoi_at)
    c["end_indices"] = len(end_at)
    return c
