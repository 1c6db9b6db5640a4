"""GPU decoding of LZW tiles (gcn10_lzw_decode.hip through gcn10_gpu_inflate_tiles) on the hand-made code
streams of tests/lzw_cases.py: every family in one launch, every byte up to out_len and every status word
against the model of tests/lzw_model.py (which tests/test_lzw_model.py holds against the host reader and
libtiff), zero guard bytes around every window.  Two families again with Predictor 2 and beside DEFLATE and raw
tiles; and what the kernel refuses before it reads a code."""
import zlib

import numpy as np
import pytest

from gcn10_amd import gpu
from tests import lzw_cases as lc
from tests.fuzz_lzw_decode import chunk_width, decode_tiles
from tests.lzw_model import CLEAR, EOI, pack

pytestmark = pytest.mark.gpu
E_HEADER, E_WINDOW = 1, 8         # GCN10_INFLATE_E_HEADER, GCN10_INFLATE_E_WINDOW (include/gcn10_gpu.h)


def _check(cases, chunks, status, want_bytes=None):
    assert len(cases) == len(chunks) == len(status)
    for i, (c, got, st) in enumerate(zip(cases, chunks, status)):
        if isinstance(c.want, bytes):
            assert int(st) == 0, (c.name, int(st))
            want = np.frombuffer(c.want if want_bytes is None else want_bytes[i], np.uint8)
            if not np.array_equal(got, want):
                first = int(np.flatnonzero(got != want)[0])
                raise AssertionError("%s: byte %d of %d is %d, not %d" % (c.name, first, c.out_len, got[first],
                                                                          want[first]))
        else:
            assert int(st) == c.want.status, (c.name, int(st), c.want.__name__)


@pytest.mark.parametrize("family", list(lc.FAMILIES))
def test_family_decodes_as_the_model_does(engine, family):
    cases = lc.FAMILIES[family]()
    assert len(cases) <= 2500
    chunks, status = decode_tiles(engine, [c.stream for c in cases], [c.out_len for c in cases])
    _check(cases, chunks, status)


def _summed(data, out_len):
    """What Predictor 2 makes of a chunk: every row of the chunk's width summed up, modulo 256."""
    cw = chunk_width(out_len)
    return np.cumsum(np.frombuffer(data, np.uint8).reshape(-1, cw), axis=1, dtype=np.uint64).astype(np.uint8).tobytes()


@pytest.mark.parametrize("family", ["chunk_end", "kwkwk"])
def test_family_with_predictor2(engine, family):
    cases = lc.FAMILIES[family]()
    chunks, status = decode_tiles(engine, [c.stream for c in cases], [c.out_len for c in cases],
                                  flags=[gpu.TILE_LZW | gpu.TILE_PREDICTOR2] * len(cases))
    _check(cases, chunks, status, [_summed(c.want, c.out_len) if isinstance(c.want, bytes) else None for c in cases])


@pytest.mark.parametrize("family", ["chunk_end", "invalid_code"])
def test_family_beside_deflate_and_raw_tiles(engine, family):
    """Every LZW tile followed by a DEFLATE tile or a raw tile of noise of about its size."""
    cases = lc.FAMILIES[family]()
    rng = np.random.default_rng(7)
    streams, lens, flags, others = [], [], [], []
    for i, c in enumerate(cases):
        data = rng.integers(0, 256 if i % 4 else 3, c.out_len, dtype=np.uint8).tobytes()
        streams += [c.stream, data if i % 2 else zlib.compress(data, 1 + i % 9)]
        lens += [c.out_len, c.out_len]
        flags += [gpu.TILE_LZW, gpu.TILE_RAW if i % 2 else 0]
        others.append(data)
    chunks, status = decode_tiles(engine, streams, lens, flags=flags)
    _check(cases, chunks[0::2], status[0::2])
    assert not status[1::2].any()
    for c, data, got in zip(cases, others, chunks[1::2]):
        assert got.tobytes() == data, c.name


def test_what_the_kernel_refuses_before_it_reads_a_code(engine):
    good = lc.kwkwk()[100]
    L, cw = good.out_len, chunk_width(good.out_len)
    rows = L // cw
    bad_first = pack([300, EOI])

    def run(stream, out_len, win, flags=gpu.TILE_LZW):
        """The tile between two good ones."""
        W, H = cw + 16, 3 * rows + 32
        out, status = engine.inflate_tiles([good.stream, stream, good.stream], cw, [rows] * 3,
                                           [(0, 0, cw, rows, 8, 8), win + (8, rows + 16), (0, 0, cw, rows, 8, 2 * rows + 24)],
                                           (H, W), flags=[gpu.TILE_LZW, flags, gpu.TILE_LZW], out_lens=[L, out_len, L])
        for y in (8, 2 * rows + 24):
            assert out[y:y + rows, 8:8 + cw].tobytes() == good.want
            out[y:y + rows, 8:8 + cw] = 0
        assert status[0] == 0 and status[2] == 0
        return out, int(status[1])

    # an empty chunk with an empty window: nothing read (not even a first code that is no literal), nothing written
    for stream in (good.stream, bad_first, b""):
        out, st = run(stream, 0, (0, 0, 0, 0))
        assert st == 0 and not out.any()
    # a window outside its chunk: to the right, below, past out_len, any window of an empty chunk
    for out_len, win in ((L, (cw - 1, 0, 2, 1)), (L, (0, rows - 1, cw, 2)), (L, (cw + 1, 0, 1, 1)), (L - 1, (0, 0, cw, rows)),
                         (0, (0, 0, 1, 1))):
        out, st = run(good.stream, out_len, win)
        assert st == E_WINDOW and not out.any(), (out_len, win)
    # the same windows inside: decoded
    out, st = run(good.stream, L, (cw - 1, rows - 1, 1, 1))
    assert st == 0 and out[rows + 16, 8] == good.want[-1] and np.count_nonzero(out) <= 1
    # LZW may not be combined with RAW
    out, st = run(good.stream, L, (0, 0, cw, rows), flags=gpu.TILE_LZW | gpu.TILE_RAW)
    assert st == E_HEADER and not out.any()
    out, st = run(pack([CLEAR, 300, EOI]), L, (0, 0, cw, rows))
    assert st == gpu.INFLATE_E_LZW_FIRST
