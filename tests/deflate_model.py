"""A plain-Python, bit-level model of zlib streams (RFC 1950 wrapper around RFC 1951 DEFLATE), CPU only.

`read(stream)` decodes a stream with zlib's own acceptance rules (inflate.c / inftrees.c of zlib 1.2.x, as
`zlib.decompress` applies them) and returns every part of it: the bytes, each block's header and code lengths,
every token, where the stream ends and whether its Adler-32 matches.  A stream zlib refuses raises `Refused`
with zlib's message.  The rules that matter most, because decoders get them wrong:
  - a code-length set may not over-subscribe the code space;
  - the precode must be complete, unless it has no code at all;
  - a literal/length or distance code may be incomplete only when it is one code of one bit;
  - a distance code with no code at all is allowed (until a distance is read);
  - the literal/length code must hold symbol 256 (end of block);
  - a repeat of the code lengths (16, 17, 18) may cross from the literal/length lengths into the distance
    lengths, but not run past HLIT + HDIST, and 16 may not come first.

`Writer` emits blocks from explicit parts (stored, fixed, dynamic with given code lengths and precode runs,
tokens with a chosen length symbol), legal or not, so that tests can build streams zlib's encoder never writes.
"""
import heapq
import zlib

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227,
         258]
LEXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
         6145, 8193, 12289, 16385, 24577]
DEXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class Refused(Exception):
    """zlib refuses the stream; str() is zlib's message."""


TRUNCATED = "incomplete or truncated stream"


class _Bits:
    def __init__(self, data):
        self.data, self.pos, self.bb, self.bc = data, 0, 0, 0

    def need(self, n):
        while self.bc < n:
            if self.pos >= len(self.data):
                raise Refused(TRUNCATED)
            self.bb |= self.data[self.pos] << self.bc
            self.pos += 1
            self.bc += 8

    def fill(self, n):
        while self.bc < n and self.pos < len(self.data):
            self.bb |= self.data[self.pos] << self.bc
            self.pos += 1
            self.bc += 8

    def bits(self, n):
        if n == 0:
            return 0
        self.need(n)
        v = self.bb & ((1 << n) - 1)
        self.bb >>= n
        self.bc -= n
        return v

    def align(self):
        self.bits(self.bc & 7)

    def bitpos(self):
        return self.pos * 8 - self.bc


def _check_lengths(lens, kind):
    """inftrees.c inflate_table: None if the set is usable, else why not.  kind: 'codes', 'lens' or 'dists'."""
    count = [0] * 16
    for n in lens:
        count[n] += 1
    count[0] = 0
    mx = max((L for L in range(1, 16) if count[L]), default=0)
    if mx == 0:
        return None                     # no code at all: a table that refuses every pattern
    left = 1
    for L in range(1, 16):
        left = 2 * left - count[L]
        if left < 0:
            return "over-subscribed"
    if left > 0 and (kind == "codes" or mx != 1):
        return "incomplete"
    return None


class _Decoder:
    """Canonical Huffman decoding by a lookup over the next `mx` bits (LSB-first as they arrive)."""

    def __init__(self, lens):
        self.mx = max(lens, default=0)
        self.empty = self.mx == 0
        if self.empty:
            return
        self.table = [None] * (1 << self.mx)
        code, nxt = 0, [0] * 17
        count = [0] * 16
        for n in lens:
            count[n] += 1
        count[0] = 0
        for L in range(1, 16):
            code = (code + count[L - 1]) << 1
            nxt[L] = code
        for sym, L in enumerate(lens):
            if not L:
                continue
            c = nxt[L]
            nxt[L] += 1
            rev = int(format(c, "0%db" % L)[::-1], 2)
            for hi in range(0, 1 << self.mx, 1 << L):
                self.table[rev | hi] = (sym, L)

    def decode(self, br, what):
        if self.empty:
            br.need(1)
            raise Refused("invalid %s code" % what)
        br.fill(self.mx)                # the bits there are, up to mx (a stream may end right after a short code)
        e = self.table[br.bb & ((1 << self.mx) - 1)]
        if e is None:
            raise Refused(TRUNCATED if br.bc < self.mx else "invalid %s code" % what)
        if e[1] > br.bc:
            raise Refused(TRUNCATED)
        br.bits(e[1])
        return e[0]


class Block:
    def __init__(self, final, btype, start_bit):
        self.final, self.type, self.start_bit = final, btype, start_bit
        self.hlit = self.hdist = self.hclen = None
        self.precode_lens = self.lit_lens = self.dist_lens = None
        self.crossing = False           # a precode run (16/17/18) crosses from the lit/len into the dist lengths
        self.cl_items = []              # the precode symbols and their extra bits
        self.tokens = []                # ('lit', byte) | ('match', length, dist, lsym, dsym) | ('eob',)
        self.stored_len = None
        self.end_bit = None


class Result:
    def __init__(self):
        self.data = b""
        self.blocks = []
        self.header = None
        self.end = None                 # bytes the stream takes, Adler-32 included
        self.adler = None               # the stream's Adler-32
        self.adler_ok = None


def _length_of(sym, br):
    k = sym - 257
    return LBASE[k] + br.bits(LEXTRA[k])


def read(stream, check_adler=True, max_out=None):
    """Decodes a zlib stream as zlib does.  Returns a Result; raises Refused(zlib's reason).  With
    check_adler=False a wrong Adler-32 is reported (adler_ok False) instead of refused."""
    stream = bytes(stream)
    br = _Bits(stream)
    res = Result()
    out = bytearray()
    cmf = br.bits(8)
    flg = br.bits(8)
    res.header = (cmf, flg)
    if (cmf << 8 | flg) % 31:
        raise Refused("incorrect header check")
    if cmf & 15 != 8:
        raise Refused("unknown compression method")
    if (cmf >> 4) + 8 > 15:
        raise Refused("invalid window size")
    if flg & 0x20:
        raise Refused("need dictionary")
    final = False
    while not final:
        start = br.bitpos()
        final = bool(br.bits(1))
        btype = br.bits(2)
        blk = Block(final, btype, start)
        res.blocks.append(blk)
        if btype == 0:
            br.align()
            ln, nln = br.bits(16), br.bits(16)
            if ln != nln ^ 0xFFFF:
                raise Refused("invalid stored block lengths")
            blk.stored_len = ln
            at = br.pos - br.bc // 8
            if at + ln > len(stream):
                raise Refused(TRUNCATED)
            out += stream[at:at + ln]
            br.pos, br.bb, br.bc = at + ln, 0, 0
            blk.end_bit = br.bitpos()
            continue
        if btype == 3:
            raise Refused("invalid block type")
        if btype == 1:
            lit_lens, dist_lens = FIXED_LIT, FIXED_DIST
        else:
            hlit, hdist, hclen = br.bits(5) + 257, br.bits(5) + 1, br.bits(4) + 4
            blk.hlit, blk.hdist, blk.hclen = hlit, hdist, hclen
            if hlit > 286 or hdist > 30:
                raise Refused("too many length or distance symbols")
            pre = [0] * 19
            for i in range(hclen):
                pre[ORDER[i]] = br.bits(3)
            blk.precode_lens = pre
            if _check_lengths(pre, "codes"):
                raise Refused("invalid code lengths set")
            pdec = _Decoder(pre)
            lens = []
            total = hlit + hdist
            while len(lens) < total:
                if pdec.empty:              # zlib's table for no code: every pattern is a 1-bit 0
                    br.bits(1)
                    sym = 0
                else:
                    sym = pdec.decode(br, "code lengths")
                if sym < 16:
                    blk.cl_items.append((sym, 0))
                    lens.append(sym)
                    continue
                if sym == 16:
                    ex = br.bits(2)
                    if not lens:
                        raise Refused("invalid bit length repeat")
                    val, rep = lens[-1], 3 + ex
                elif sym == 17:
                    ex = br.bits(3)
                    val, rep = 0, 3 + ex
                else:
                    ex = br.bits(7)
                    val, rep = 0, 11 + ex
                blk.cl_items.append((sym, ex))
                if len(lens) + rep > total:
                    raise Refused("invalid bit length repeat")
                if len(lens) < hlit < len(lens) + rep:
                    blk.crossing = True
                lens += [val] * rep
            lit_lens, dist_lens = lens[:hlit], lens[hlit:]
            if lit_lens[256] == 0:
                raise Refused("invalid code -- missing end-of-block")
            if _check_lengths(lit_lens, "lens"):
                raise Refused("invalid literal/lengths set")
            if _check_lengths(dist_lens, "dists"):
                raise Refused("invalid distances set")
        blk.lit_lens, blk.dist_lens = list(lit_lens), list(dist_lens)
        ldec, ddec = _Decoder(lit_lens), _Decoder(dist_lens)
        toks = blk.tokens
        while True:
            sym = ldec.decode(br, "literal/length")
            if sym < 256:
                out.append(sym)
                toks.append(("lit", sym))
            elif sym == 256:
                toks.append(("eob",))
                break
            else:
                if sym > 285:
                    raise Refused("invalid literal/length code")
                length = _length_of(sym, br)
                dsym = ddec.decode(br, "distance")
                if dsym > 29:
                    raise Refused("invalid distance code")
                dist = DBASE[dsym] + br.bits(DEXTRA[dsym])
                if dist > len(out):
                    raise Refused("invalid distance too far back")
                toks.append(("match", length, dist, sym, dsym))
                s = len(out) - dist
                for k in range(length):
                    out.append(out[s + k])
            if max_out is not None and len(out) > max_out:
                raise ValueError("stream decodes to more than %d bytes" % max_out)
        blk.end_bit = br.bitpos()
    br.align()
    at = br.pos - br.bc // 8
    if at + 4 > len(stream):
        raise Refused(TRUNCATED)
    adler = int.from_bytes(stream[at:at + 4], "big")
    br.pos, br.bb, br.bc = at + 4, 0, 0
    res.data = bytes(out)
    res.end = br.pos
    res.adler = adler
    res.adler_ok = adler == zlib.adler32(res.data)
    if check_adler and not res.adler_ok:
        raise Refused("incorrect data check")
    return res


def zlib_verdict(stream):
    """(bytes, None) when zlib.decompress accepts the stream, (None, zlib's reason) when it refuses it."""
    try:
        return zlib.decompress(bytes(stream)), None
    except zlib.error as e:
        msg = str(e)
        return None, msg.split(": ", 1)[1] if ": " in msg else msg


def model_verdict(stream):
    try:
        return read(stream).data, None
    except Refused as e:
        return None, str(e)


# ---------------------------------------------------------------------------------------------------- writer

def huffman_depths(freqs):
    """Code lengths of an unconstrained Huffman code of the nonzero frequencies (one used symbol: length 1)."""
    live = [(f, i) for i, f in enumerate(freqs) if f]
    depth = [0] * len(freqs)
    if not live:
        return depth
    if len(live) == 1:
        depth[live[0][1]] = 1
        return depth
    heap = [(f, k, [i]) for k, (f, i) in enumerate(live)]
    heapq.heapify(heap)
    k = len(heap)
    while len(heap) > 1:
        f1, _, a = heapq.heappop(heap)
        f2, _, b = heapq.heappop(heap)
        for i in a + b:
            depth[i] += 1
        heapq.heappush(heap, (f1 + f2, k, a + b))
        k += 1
    return depth


def limited_lengths(freqs, limit):
    """Optimal code lengths of at most `limit` bits (package-merge); a complete code when two or more symbols are
    used, one 1-bit code when one is."""
    live = sorted((f, i) for i, f in enumerate(freqs) if f)
    out = [0] * len(freqs)
    if not live:
        return out
    if len(live) == 1:
        out[live[0][1]] = 1
        return out
    assert len(live) <= 1 << limit
    leaves = [(f, (i,)) for f, i in live]
    pk = list(leaves)
    for _ in range(limit - 1):
        pairs = [(pk[j][0] + pk[j + 1][0], pk[j][1] + pk[j + 1][1]) for j in range(0, len(pk) - 1, 2)]
        pk = sorted(leaves + pairs, key=lambda t: t[0])
    for _, syms in pk[:2 * len(live) - 2]:
        for i in syms:
            out[i] += 1
    return out


def code_words(lens):
    """Canonical codes (RFC 1951 3.2.2): symbol -> (code, length)."""
    count = [0] * 16
    for n in lens:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for L in range(1, 16):
        code = (code + count[L - 1]) << 1
        nxt[L] = code
    words = {}
    for s, L in enumerate(lens):
        if L:
            words[s] = (nxt[L], L)
            nxt[L] += 1
    return words


def length_symbol(length):
    if length == 258:
        return 285
    return 257 + max(k for k in range(28) if LBASE[k] <= length)


def dist_symbol(dist):
    return max(k for k in range(30) if DBASE[k] <= dist)


def rle_lengths(seq):
    """Precode items (symbol, extra) for a sequence of code lengths, greedy, runs as long as they go (so they
    cross from the literal/length into the distance lengths when given both as one sequence)."""
    items, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                n = min(run, 138)
                items.append((18, n - 11))
                run -= n
            if run >= 3:
                items.append((17, run - 3))
                run = 0
            items += [(0, 0)] * run
        else:
            items.append((v, 0))
            run -= 1
            while run >= 3:
                n = min(run, 6)
                items.append((16, n - 3))
                run -= n
            items += [(v, 0)] * run
        i = j
    return items


_EXTRA_BITS = {16: 2, 17: 3, 18: 7}


class Writer:
    """Builds a zlib stream block by block.  `raw` follows the bytes the tokens produce (None once a token reads
    before the start, as an invalid stream may)."""

    def __init__(self, header=b"\x78\x9c"):
        self.out = bytearray(header)
        self.acc = self.n = 0
        self.raw = bytearray()

    def bits(self, v, n):
        assert 0 <= v < (1 << n) or n == 0
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, word):
        c, n = word
        self.bits(int(format(c, "0%db" % n)[::-1], 2), n)

    def bitpos(self):
        return len(self.out) * 8 + self.n

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def stored(self, data, final=False, nlen=None):
        self.bits(int(final), 1)
        self.bits(0, 2)
        self.align()
        data = bytes(data)
        self.bits(len(data), 16)
        self.bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
        self.out += data
        if self.raw is not None:
            self.raw += data

    def _tokens(self, tokens, lw, dw):
        """tokens: an int (literal), ('match', length, dist[, lsym]), ('sym', lsym, extra[, dsym, dextra]) for any
        symbol at all; the end of block is written by the caller."""
        for t in tokens:
            if isinstance(t, int):
                self.code(lw[t])
                if self.raw is not None:
                    self.raw.append(t)
            elif t[0] == "match":
                length, dist = t[1], t[2]
                lsym = t[3] if len(t) > 3 else length_symbol(length)
                k = lsym - 257
                assert 0 <= length - LBASE[k] < 1 << LEXTRA[k] or (k == 28 and length == 258), (length, lsym)
                self.code(lw[lsym])
                self.bits(length - LBASE[k], LEXTRA[k])
                d = dist_symbol(dist)
                self.code(dw[d])
                self.bits(dist - DBASE[d], DEXTRA[d])
                if self.raw is not None:
                    if dist > len(self.raw):
                        self.raw = None
                    else:
                        for _ in range(length):
                            self.raw.append(self.raw[-dist])
            elif t[0] == "sym":
                self.code(lw[t[1]])
                if len(t) > 2:
                    self.bits(t[2], LEXTRA[t[1] - 257] if 257 <= t[1] <= 285 else 0)
                if len(t) > 3:
                    self.code(dw[t[3]])
                    self.bits(t[4], DEXTRA[t[3]] if t[3] < 30 else 0)
                self.raw = None
            else:
                raise ValueError(t)

    def fixed(self, tokens, final=False, eob=True):
        self.bits(int(final), 1)
        self.bits(1, 2)
        lw, dw = code_words(FIXED_LIT), code_words(FIXED_DIST)
        self._tokens(tokens, lw, dw)
        if eob:
            self.code(lw[256])

    def dynamic(self, tokens, final=False, lit_lens=None, dist_lens=None, hlit=None, hdist=None, hclen=None,
                items=None, precode_lens=None, eob=True, cross=True):
        """A dynamic block.  Code lengths default to a 15-bit limited Huffman code of the tokens' counts (with
        symbol 256 counted once); the code-length sequence is run-length coded as one sequence (cross=True: its
        runs may cross HLIT) or as two; the precode defaults to a 7-bit limited code of its items' counts.  Every
        part can be given instead: hlit / hdist / hclen are the counts the header announces."""
        lf, df = [0] * 288, [0] * 32
        lf[256] = 1 if eob else 0
        for t in tokens:
            if isinstance(t, int):
                lf[t] += 1
            elif t[0] == "match":
                lf[t[3] if len(t) > 3 else length_symbol(t[1])] += 1
                df[dist_symbol(t[2])] += 1
        if lit_lens is None:
            lit_lens = limited_lengths(lf[:286], 15)
        if dist_lens is None:
            dist_lens = limited_lengths(df[:30], 15)
        lit_lens, dist_lens = list(lit_lens), list(dist_lens)
        if hlit is None:
            hlit = max(257, max((i + 1 for i, L in enumerate(lit_lens) if L), default=0))
        if hdist is None:
            hdist = max(1, max((i + 1 for i, L in enumerate(dist_lens) if L), default=0))
        ll = (lit_lens + [0] * 288)[:hlit]
        dl = (dist_lens + [0] * 32)[:hdist]
        if items is None:
            items = rle_lengths(ll + dl) if cross else rle_lengths(ll) + rle_lengths(dl)
        if precode_lens is None:
            pf = [0] * 19
            for s, _ in items:
                pf[s] += 1
            precode_lens = limited_lengths(pf, 7)
        if hclen is None:
            hclen = max([4] + [i + 1 for i in range(19) if precode_lens[ORDER[i]]])
        self.bits(int(final), 1)
        self.bits(2, 2)
        self.bits(hlit - 257, 5)
        self.bits(hdist - 1, 5)
        self.bits(hclen - 4, 4)
        for i in range(hclen):
            self.bits(precode_lens[ORDER[i]], 3)
        pw = code_words(precode_lens)
        for s, ex in items:
            self.code(pw[s])
            if s >= 16:
                self.bits(ex, _EXTRA_BITS[s])
        lw, dw = code_words(ll), code_words(dl)
        self._tokens(tokens, lw, dw)
        if eob:
            self.code(lw[256])

    def raw_bits(self, v, n):
        self.bits(v, n)

    def finish(self, adler=None):
        """The stream with its Adler-32 (of the bytes the tokens produced, unless given)."""
        self.align()
        if adler is None:
            adler = zlib.adler32(bytes(self.raw)) if self.raw is not None else 1
        return bytes(self.out) + adler.to_bytes(4, "big")
