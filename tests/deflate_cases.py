"""Hand-made zlib streams in the forms zlib's encoder never writes, legal and not (tests/deflate_model.py Writer).

valid_cases()   -> [(name, stream, bytes)]: streams zlib accepts
invalid_cases() -> [(name, stream, zlib's reason, GCN10_INFLATE_E_* the GPU decoder must report)]
Shared by the CPU model test (zlib's verdict) and the GPU decoder test."""
import numpy as np

from tests.deflate_model import DBASE, Writer

E_BLOCK_TYPE, E_STORED, E_LENGTHS, E_CODE, E_DISTANCE = 2, 3, 4, 5, 6


def _lens(n, assign):
    out = [0] * n
    for s, L in assign.items():
        out[s] = L
    return out


def _rand(n, seed, hi=256):
    return [int(v) for v in np.random.default_rng(seed).integers(0, hi, n)]


def _crossing_16():
    # lit 280..285 and dist 0..15 all 4 bits: one run of 22 fours, coded 4 + 16 x3 + ..., crosses HLIT = 286
    lit = _lens(286, {97: 2, 98: 2, 256: 3, **{s: 4 for s in range(280, 286)}})
    dist = [4] * 16
    w = Writer()
    toks = [97, 98] * 150
    for k, (length, lsym) in enumerate([(120, 280), (140, 281), (170, 282), (200, 283), (240, 284), (258, 285)]):
        toks += [("match", length, 193 + 9 * k, lsym), 97, 98]
        toks += [("match", length if lsym == 285 else length - 5, DBASE[2 * k + 1], lsym)]
    w.dynamic(toks, final=True, lit_lens=lit, dist_lens=dist, hlit=286, hdist=16)
    return w


def _crossing_zeros(hlit, hdist, dist_assign, lsym, length):
    # literal/length lengths end in zeros that run on into the distance lengths (17 for a short run, 18 for a long one)
    lit = _lens(hlit, {97: 2, 98: 2, 256: 2, lsym: 2})
    dist = _lens(hdist, dist_assign)
    d = sorted(dist_assign)
    toks = [97, 98] * 80
    for k in range(12):
        toks += [("match", length, DBASE[d[k % len(d)]] + k % 2, lsym), 98]
    w = Writer()
    w.dynamic(toks, final=True, lit_lens=lit, dist_lens=dist, hlit=hlit, hdist=hdist)
    return w


def _fifteen_bit_codes():
    # lengths 1..15, 15: the precode uses symbol 15 (HCLEN 19), literal/length and distance codes reach 15 bits
    lsyms = list(range(13)) + [257, 256, 13]
    lit = _lens(258, {s: L for s, L in zip(lsyms, list(range(1, 15)) + [15, 15])})
    dist = _lens(16, {s: L for s, L in zip(range(16), list(range(1, 15)) + [15, 15])})
    toks = list(range(14)) * 20
    for k in range(40):
        toks += [13, 12, ("match", 3, DBASE[15] + k, 257), ("match", 3, DBASE[14] + k, 257), 13]
    w = Writer()
    w.dynamic(toks, final=True, lit_lens=lit, dist_lens=dist)
    return w


def valid_cases():
    cases = []

    def add(name, w):
        cases.append((name, w.finish(), bytes(w.raw)))

    add("crossing_16", _crossing_16())
    add("crossing_17", _crossing_zeros(263, 6, {4: 1, 5: 1}, 260, 6))
    add("crossing_18", _crossing_zeros(286, 12, {10: 1, 11: 1}, 260, 6))
    add("fifteen_bit_codes_hclen19", _fifteen_bit_codes())

    # HLIT 257 (literals and the end of block only) with a distance code of no symbol at all
    w = Writer()
    data = _rand(3000, 1)
    lit = [8] * 257                             # 255 codes of 8 bits and 2 of 9: complete
    lit[255], lit[256] = 9, 9
    w.dynamic(data, final=True, lit_lens=lit, hlit=257, dist_lens=[0], hdist=1)
    add("hlit257_no_distance_code", w)

    # HLIT 286 and a distance code of ONE symbol (one 1-bit code, incomplete: legal)
    w = Writer()
    toks = [97, 98, 99] * 50 + [("match", 258, 2, 285), ("match", 10, 2)] * 5
    lit = _lens(286, {97: 2, 98: 2, 99: 3, 256: 3, 264: 3, 285: 3})
    w.dynamic(toks, final=True, lit_lens=lit, hlit=286, dist_lens=[0, 1], hdist=2)
    add("hlit286_one_distance_code", w)

    # HCLEN 5: only 16 17 18 0 8 in the precode -- 255 literals of 8 bits, the end of block 8 bits
    w = Writer()
    lit = [8] * 256 + [8]
    lit[255] = 0
    w.dynamic([b for b in _rand(2000, 2) if b != 255], final=True, lit_lens=lit, hlit=257, dist_lens=[0], hdist=1)
    add("hclen5", w)

    # blocks whose code holds only the end of block; empty fixed, stored and dynamic blocks
    w = Writer()
    w.dynamic([], lit_lens=_lens(257, {256: 1}), hlit=257, dist_lens=[0], hdist=1)
    w.fixed([])
    w.stored(b"")
    w.fixed([1, 2, 3])
    w.dynamic([], lit_lens=_lens(257, {256: 1}), hlit=257, dist_lens=[0], hdist=1)
    w.stored(b"", final=True)
    add("only_end_of_block_and_empty_blocks", w)

    w = Writer()
    w.fixed([], final=True)
    add("empty_stream", w)

    # length 258 as 285 and as 284 + 31 extra bits; length-3 matches more than 4096 back
    w = Writer()
    base = _rand(9000, 3)
    toks = [("match", 258, 1, 284), ("match", 258, 1, 285), ("match", 258, 700, 284), ("match", 227, 5000, 284)]
    for k in range(30):
        toks += [("match", 3, 4097 + 123 * k), 7, ("match", 3, 8000 + k)]
    w.fixed(base)
    w.dynamic(toks, final=True)
    add("length_258_two_ways_and_far_3s", w)

    # distance exactly 32768, sources in earlier blocks (stored, fixed, dynamic), a 65535-byte stored block
    w = Writer()
    big = bytes(_rand(65535, 4))
    w.stored(big)
    w.fixed([("match", 258, 32768), ("match", 3, 32768), 5, ("match", 100, 32768), ("match", 258, 32767)])
    w.stored(b"")
    w.dynamic([("match", 258, 32768)] * 3 + [("match", 31, 30000), ("match", 4, 1)] + _rand(50, 5), final=True)
    add("distance_32768_across_blocks_stored_65535", w)

    # every block boundary at every bit offset mod 32 (a non-final fixed block of m 9-bit literals, then a final one
    # whose end of block lands at every offset as well)
    for m in range(33):
        w = Writer()
        w.fixed([200] * m + [("match", 3, 1)] * (m > 0))
        w.fixed([150 + (m % 7)] * (m + 5) + [10, ("match", 4, 2)], final=True)
        add("end_of_block_after_%d_literals" % m, w)
    return cases


def invalid_cases():
    cases = []

    def add(name, w, reason, code, adler=None):
        cases.append((name, w.finish(adler), reason, code))

    two_lit = _lens(257, {97: 1, 256: 1})
    # incomplete codes
    w = Writer()
    w.dynamic([97, 98], final=True, lit_lens=_lens(257, {97: 2, 98: 2, 256: 2}), dist_lens=[1, 1])
    add("incomplete_literal_length_code", w, "invalid literal/lengths set", E_LENGTHS)
    w = Writer()
    w.dynamic([97, 97, 97, ("match", 3, 1)], final=True, lit_lens=_lens(258, {97: 1, 256: 2, 257: 2}),
              dist_lens=[2, 2, 2])
    add("incomplete_distance_code", w, "invalid distances set", E_LENGTHS)
    w = Writer()
    w.dynamic([97], final=True, lit_lens=two_lit, dist_lens=[1, 1], hlit=257, hdist=2,
              precode_lens=_lens(19, {0: 2, 1: 2, 18: 2}))
    add("incomplete_precode", w, "invalid code lengths set", E_LENGTHS)
    w = Writer()
    w.dynamic([97], final=True, lit_lens=two_lit, dist_lens=[0], hdist=1, items=[(1, 0)] * 258,
              precode_lens=_lens(19, {1: 1}))
    add("precode_of_one_1bit_code", w, "invalid code lengths set", E_LENGTHS)
    # over-subscribed codes
    w = Writer()
    w.dynamic([97], final=True, lit_lens=_lens(257, {97: 1, 98: 1, 256: 1}), dist_lens=[1, 1])
    add("oversubscribed_literal_length_code", w, "invalid literal/lengths set", E_LENGTHS)
    w = Writer()
    w.dynamic([97], final=True, lit_lens=two_lit, dist_lens=[1, 1, 1])
    add("oversubscribed_distance_code", w, "invalid distances set", E_LENGTHS)
    w = Writer()
    w.dynamic([97], final=True, lit_lens=two_lit, dist_lens=[1, 1], precode_lens=_lens(19, {0: 1, 1: 1, 18: 1}))
    add("oversubscribed_precode", w, "invalid code lengths set", E_LENGTHS)
    # no end-of-block code
    w = Writer()
    w.dynamic([97, 98], final=True, lit_lens=_lens(257, {97: 1, 98: 1}), dist_lens=[1, 1], hlit=257, eob=False)
    add("missing_end_of_block_code", w, "invalid code -- missing end-of-block", E_LENGTHS)
    w = Writer()
    w.dynamic([], final=True, lit_lens=[0] * 257, dist_lens=[0], hlit=257, hdist=1, hclen=4, eob=False,
              precode_lens=_lens(19, {0: 1, 18: 1}))
    add("hclen4_no_lengths_at_all", w, "invalid code -- missing end-of-block", E_LENGTHS)
    # header counts
    for hlit, hdist in ((287, 2), (288, 2), (257, 31), (257, 32)):
        w = Writer()
        w.dynamic([97], final=True, lit_lens=two_lit, dist_lens=[1, 1], hlit=hlit, hdist=hdist)
        add("hlit%d_hdist%d" % (hlit, hdist), w, "too many length or distance symbols", E_LENGTHS)
    # repeats
    w = Writer()
    w.dynamic([97], final=True, lit_lens=two_lit, dist_lens=[1, 1], items=[(16, 0), (0, 0)] + [(0, 0)] * 257)
    add("leading_16", w, "invalid bit length repeat", E_LENGTHS)
    w = Writer()
    items = [(0, 0)] * 97 + [(1, 0)] + [(18, 127)] + [(0, 0)] * 19 + [(1, 0), (1, 0), (18, 0)]
    w.dynamic([97], final=True, lit_lens=two_lit, dist_lens=[1, 1], hlit=257, hdist=2, items=items)
    add("run_past_hlit_plus_hdist", w, "invalid bit length repeat", E_LENGTHS)
    # symbols a fixed block may not use
    for lsym in (286, 287):
        w = Writer()
        w.fixed([1, 2, 3, ("sym", lsym)], final=True)
        add("fixed_symbol_%d" % lsym, w, "invalid literal/length code", E_CODE)
    for dsym in (30, 31):
        w = Writer()
        w.fixed([1, 2, 3, ("sym", 257, 0, dsym, 0)], final=True)
        add("fixed_distance_%d" % dsym, w, "invalid distance code", E_CODE)
    # a distance code of no symbol, or of one 1-bit code, read where it has none; the other half of a one-code
    # literal/length code
    w = Writer()
    w.dynamic([97, 97, 97, ("sym", 257, 0)], final=True, lit_lens=_lens(258, {97: 1, 256: 2, 257: 2}),
              dist_lens=[0], hdist=1)
    w.raw_bits(0, 8)
    add("distance_of_an_empty_distance_code", w, "invalid distance code", E_CODE)
    w = Writer()
    w.dynamic([97, 97, 97, ("sym", 257, 0)], final=True, lit_lens=_lens(258, {97: 1, 256: 2, 257: 2}),
              dist_lens=[1], hdist=1)
    w.raw_bits(1, 1)                            # the 1-bit pattern that is no code
    add("missing_half_of_a_one_code_distance_code", w, "invalid distance code", E_CODE)
    w = Writer()
    w.dynamic([], final=True, lit_lens=_lens(257, {256: 1}), dist_lens=[0], hdist=1, eob=False)
    w.raw_bits(1, 1)
    add("missing_half_of_a_one_code_literal_length_code", w, "invalid literal/length code", E_CODE)
    # the rest
    w = Writer()
    w.fixed([1, 2, 3, ("match", 5, 4)], final=True)
    add("distance_too_far_back", w, "invalid distance too far back", E_DISTANCE)
    w = Writer()
    w.fixed(list(range(40)) * 3)
    w.fixed([("match", 10, 200)], final=True)
    add("distance_too_far_back_in_a_later_block", w, "invalid distance too far back", E_DISTANCE)
    w = Writer()
    w.fixed([1, 2, 3])
    w.raw_bits(1, 1)
    w.raw_bits(3, 2)
    w.raw_bits(0, 29)
    add("block_type_3", w, "invalid block type", E_BLOCK_TYPE)
    w = Writer()
    w.stored(b"abcde", final=True, nlen=0xFFFA ^ 0x0100)
    add("bad_nlen", w, "invalid stored block lengths", E_STORED)
    return cases
