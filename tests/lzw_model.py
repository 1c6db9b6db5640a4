"""A model of TIFF LZW decoding for the tests of the GPU LZW decoder (gcn10_lzw_decode.hip) and of the host
reader (tiff_codec.c lzw_decode): a reference decoder that can say what every code did, and a writer of code
streams in which the test chooses every code.

The semantics are those of tiff_codec.c lzw_decode (TIFF 6.0 section 13 as libtiff reads it): MSB-first codes of
9..12 bits with the early change of the width, ClearCode 256, EndOfInformation 257, KwKwK (code == next), a
dictionary that stops growing at 4096 entries, `cap` bytes out: the code that reaches cap is the last one read
and is cut there, an early EOI leaves zeros.  Three things fail, each with its own exception, which carries
the status word the GPU decoder reports for it."""
import collections

CLEAR, EOI, FIRST, MAXC = 256, 257, 258, 4096


class LzwError(ValueError):
    status = None


class LzwCodeError(LzwError):
    """a code beyond the dictionary (GCN10_INFLATE_E_LZW_CODE)"""
    status = 9


class LzwFirstError(LzwError):
    """a first code, of the stream or after a Clear, that is not a literal (GCN10_INFLATE_E_LZW_FIRST)"""
    status = 10


class LzwInputError(LzwError):
    """input that ends without EOI before cap bytes (GCN10_INFLATE_E_LZW_INPUT)"""
    status = 11


def width_of(n):
    """Bits of the n-th code after a Clear (or the start): next = 257 + n reaches 511, 1023, 2047 one code
    early."""
    return 9 if n < 254 else 10 if n < 766 else 11 if n < 1790 else 12


def pack(codes):
    """MSB-first bit packing of a code sequence at the widths the decoder reads them (early change)."""
    acc, nbits, out, n = 0, 0, bytearray(), 0
    for c in codes:
        w = width_of(n)
        assert 0 <= c < (1 << w), (c, w)
        acc = (acc << w) | c
        nbits += w
        while nbits >= 8:
            out.append((acc >> (nbits - 8)) & 0xFF)
            nbits -= 8
        acc &= (1 << nbits) - 1
        n = 0 if c == CLEAR else n + 1
    if nbits:
        out.append((acc << (8 - nbits)) & 0xFF)
    return bytes(out)


# one data code: index = codes since the last Clear (or the start), width = bits read, pos = output position of
# its first byte, length of its string, literal = the byte or None, source = output position where its string
# first lay (None for a literal; for KwKwK the start of the previous code), cut = cap fell inside its string,
# code = its value
Code = collections.namedtuple("Code", "index width pos length literal source kwkwk cut code")
# a Clear or an EOI: index = data codes since the last Clear before it, width = bits read, bit = where it starts
Mark = collections.namedtuple("Mark", "index width bit pos")


class Trace:
    def __init__(self):
        self.codes, self.clears, self.eois = [], [], []
        self.end = None         # "cap", "eoi", "input" (ended on the last byte with cap reached)
        self.bits_read = 0


def lzw_decode_ref(src, cap, trace=False):
    """cap bytes out (zeros after an early EOI), codes after cap bytes ignored; LzwCodeError, LzwFirstError
    or LzwInputError where it fails.  An empty chunk (cap == 0) reads no code at all.  With trace=True
    returns (bytes, Trace)."""
    tr = Trace()
    out = bytearray()
    table = [bytes([i]) for i in range(256)] + [b"", b""]
    starts = []                 # output position of the n-th code since the Clear
    width, prev = 9, None
    bits = nbits = ip = 0

    def done(end):
        tr.end = end
        tr.bits_read = 8 * ip - nbits
        data = bytes(out[:cap]) + bytes(max(0, cap - len(out)))
        return (data, tr) if trace else data

    if cap == 0:
        return done("cap")
    while True:
        while nbits < width:
            if ip >= len(src):
                if len(out) >= cap:
                    return done("input")
                raise LzwInputError("input ended without EOI")
            bits = (bits << 8) | src[ip]
            ip += 1
            nbits += 8
        code = (bits >> (nbits - width)) & ((1 << width) - 1)
        nbits -= width
        bits &= (1 << nbits) - 1
        if code == EOI:
            tr.eois.append(Mark(len(starts), width, 8 * ip - nbits - width, len(out)))
            return done("eoi")
        if code == CLEAR:
            tr.clears.append(Mark(len(starts), width, 8 * ip - nbits - width, len(out)))
            del table[FIRST:]
            starts = []
            width, prev = 9, None
            continue
        pos = len(out)
        if prev is None:
            if code >= 256:
                raise LzwFirstError("first code is not a literal")
            s, source, kw = table[code], None, False
        else:
            nxt = len(table)
            if code > nxt:
                raise LzwCodeError("code beyond the dictionary")
            kw = code == nxt
            s = table[prev] + table[prev][:1] if kw else table[code]
            source = None if code < 256 else starts[-1] if kw else starts[code - FIRST]
            if nxt < MAXC:
                table.append(table[prev] + s[:1])
        if trace:
            tr.codes.append(Code(len(starts), width, pos, len(s), code if code < 256 else None, source, kw,
                                 pos + len(s) > cap, code))
        out += s
        starts.append(pos)
        if prev is not None and len(table) + 1 >= (1 << width) and width < 12:
            width += 1
        prev = code
        if len(out) >= cap:
            return done("cap")


class LzwWriter:
    """A code stream written one chosen code at a time.  It keeps the dictionary a decoder has after the
    codes so far, so it knows which codes are live and which bytes they give (`out`).  raw() appends a code
    unchecked, for streams a decoder must refuse; after it `out` no longer follows."""

    def __init__(self, clear=True):
        self.codes, self.out = [], bytearray()
        self._reset()
        if clear:
            self.clear()

    def _reset(self):
        self.table = [bytes([i]) for i in range(256)] + [b"", b""]
        self.prev, self.n = None, 0
        self.starts = []        # output position of every code since the Clear

    def source(self, entry):
        """Output position where the string of a live entry first lay."""
        return self.starts[entry - FIRST]

    @property
    def next(self):
        """The code a KwKwK would have now; the live entries are FIRST .. next - 1."""
        return len(self.table)

    @property
    def full(self):
        return len(self.table) >= MAXC

    def string(self, code):
        return self.table[code]

    def code(self, c):
        """A literal, a live entry or (c == next) KwKwK; returns the length of its string."""
        if self.prev is None:
            assert c < 256, "the first code after a Clear is a literal"
            s = self.table[c]
        else:
            n = len(self.table)
            assert c <= n and c not in (CLEAR, EOI) and (c < n or n < MAXC), (c, n)
            s = self.table[self.prev] + self.table[self.prev][:1] if c == n else self.table[c]
            if n < MAXC:
                self.table.append(self.table[self.prev] + s[:1])
        self.starts.append(len(self.out))
        self.out += s
        self.prev = c
        self.n += 1
        self.codes.append(c)
        return len(s)

    def lit(self, b):
        return self.code(b)

    def kwkwk(self):
        assert self.prev is not None and not self.full
        return self.code(len(self.table))

    def newest(self, back=0):
        """The entry made `back` codes ago (0 = by the last code)."""
        assert len(self.table) - 1 - back >= FIRST
        return self.code(len(self.table) - 1 - back)

    def clear(self):
        self.codes.append(CLEAR)
        self._reset()

    def eoi(self):
        self.codes.append(EOI)

    def raw(self, c):
        self.codes.append(c)
        self.n += 1

    def stream(self):
        return pack(self.codes)
