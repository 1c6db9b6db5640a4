"""GPU zlib decoding (gcn10_gpu_inflate_tiles) of the forms zlib's encoder never writes: hand-made streams of
tests/deflate_cases.py and the libdeflate corpus of tests/golden/deflate/, checked against the zlib model of
tests/deflate_model.py.  Valid streams decode byte for byte; a stream zlib refuses gets the specific
GCN10_INFLATE_E_* status; a landcover tile zlib refuses fails its block on the GPU route as on the host route."""
import hashlib
import json
import os
import zlib

import numpy as np
import pytest
from PIL import Image

from gcn10_amd import gpu
from tests import deflate_cases as dc
from tests import deflate_model as dm
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
CW = 1024


@pytest.fixture(scope="module")
def engine():
    with gpu.Engine(0) as e:
        yield e


def _decode(engine, streams, sizes):
    """Every stream one chunk CW wide with at least one row more than its bytes need, so that the decoder reads
    on to the final end of block (the bytes past the end stay zero, as in the host reader).  One launch."""
    rows = [s // CW + 1 for s in sizes]
    ys = np.concatenate([[0], np.cumsum(rows)]).astype(int)
    wins = [(0, 0, CW, rows[i], 0, int(ys[i])) for i in range(len(streams))]
    out, status = engine.inflate_tiles(streams, CW, rows, wins, (int(ys[-1]), CW))
    return [out[ys[i]:ys[i + 1]].reshape(-1) for i in range(len(streams))], status


def test_crafted_valid_streams_decode_as_zlib_decodes_them(engine):
    cases = dc.valid_cases()
    chunks, status = _decode(engine, [st for _, st, _ in cases], [len(raw) for _, _, raw in cases])
    for (name, st, raw), got, s in zip(cases, chunks, status):
        assert dm.read(st).data == raw
        assert int(s) == 0, name
        assert got[:len(raw)].tobytes() == raw, name
        assert not got[len(raw):].any(), name


def test_crafted_valid_streams_of_exact_size(engine):
    """The same streams in chunks of exactly their size (one row): the decoder stops at the last byte."""
    for name, st, raw in dc.valid_cases():
        if not raw:
            continue
        out, status = engine.inflate_tiles([st], len(raw), [1], [(0, 0, len(raw), 1, 0, 0)], (1, len(raw)))
        assert int(status[0]) == 0 and out.tobytes() == raw, name


def test_crafted_invalid_streams_get_their_status(engine):
    cases = dc.invalid_cases()
    _, status = _decode(engine, [st for _, st, _, _ in cases], [4096] * len(cases))
    got = {name: int(s) for (name, _, _, _), s in zip(cases, status)}
    want = {name: code for name, _, _, code in cases}
    assert got == want


def test_a_wrong_checksum_is_not_checked(engine):
    """Out of scope on purpose: the GPU decoder does not verify Adler-32 (zlib's uncompress() does), so a stream
    whose only fault is its checksum decodes to its bytes."""
    raw = np.repeat(np.arange(40, dtype=np.uint8), 97).tobytes()
    st = zlib.compress(raw, 6)
    bad = st[:-4] + (int.from_bytes(st[-4:], "big") ^ 0x5A5A).to_bytes(4, "big")
    assert dm.zlib_verdict(bad) == (None, "incorrect data check")
    assert dm.read(bad, check_adler=False).data == raw
    chunks, status = _decode(engine, [bad, bad[:-4]], [len(raw)] * 2)
    assert not status.any()
    assert chunks[0][:len(raw)].tobytes() == raw and chunks[1][:len(raw)].tobytes() == raw


def test_the_libdeflate_corpus_decodes_at_its_tile_size(engine):
    corpus = os.path.join(GOLDEN, "deflate")
    with open(os.path.join(corpus, "manifest.json")) as f:
        man = json.load(f)
    for width in sorted({e["width"] for e in man}):
        part = [e for e in man if e["width"] == width]
        streams = []
        for e in part:
            with open(os.path.join(corpus, e["file"]), "rb") as f:
                streams.append(f.read())
        rows = [e["rows"] for e in part]
        ys = np.concatenate([[0], np.cumsum(rows)]).astype(int)
        wins = [(0, 0, width, rows[i], 0, int(ys[i])) for i in range(len(part))]
        out, status = engine.inflate_tiles(streams, width, rows, wins, (int(ys[-1]), width))
        assert not status.any(), [(e["file"], int(s)) for e, s in zip(part, status) if s]
        for i, e in enumerate(part):
            got = out[ys[i]:ys[i + 1]].tobytes()
            assert len(got) == e["size"] and hashlib.sha256(got).hexdigest() == e["sha256"], e["file"]


def test_tile_with_an_incomplete_code_fails_its_block_on_both_routes(tmp_path, tables):
    """A landcover tile whose literal/length code is incomplete: zlib (the host reader's uncompress()) refuses it,
    and so must the GPU decoder -- before, it decoded such a tile to whatever its codes gave."""
    from tests.test_cli import BLOCKS, _check_block, _run, _world
    name, st, reason, code = [c for c in dc.invalid_cases() if c[0] == "incomplete_literal_length_code"][0]
    assert code == dc.E_LENGTHS and dm.zlib_verdict(st) == (None, reason)
    for gpu_on in (1, 0):
        d = tmp_path / ("gpu" if gpu_on else "host")
        d.mkdir()
        esa, soil = _world(d, seed=84, extra_cfg="gpu_inflate=%d\n" % gpu_on)
        path = d / "esa.tif"
        raw = bytearray(path.read_bytes())
        im = Image.open(str(path))
        assert im.tag_v2[259] == 8
        offs, cnts = im.tag_v2[324], im.tag_v2[325]
        k = 2 * ((3000 + 511) // 512) + 3                    # tile (row 2, col 3): block 102 only
        assert cnts[k] > len(st)
        raw[offs[k]:offs[k] + cnts[k]] = st + bytes(cnts[k] - len(st))
        path.write_bytes(bytes(raw))
        (d / "ids.txt").write_text("101 102\n")
        out = _run(d, "-c", "config.txt", "-l", "ids.txt")
        assert out.returncode == 0, out.stderr[-2000:]
        log = (d / "logs" / "rank_0.log").read_text()
        assert "gdalrasterio error: cannot decode a tile of the window" in log
        assert "[ERROR] [rank 0] esa load failed for block 102" in log
        assert not (d / "cn_rasters_drained" / "cn_p_i_102.tif").exists()
        _check_block(d, esa, soil, tables, 101, BLOCKS[0][1:])
        line = [ln for ln in log.splitlines() if "timing: landcover windows:" in ln]
        assert len(line) == 1
        assert ("2 through the gpu decoder" if gpu_on else "0 through the gpu decoder") in line[0], line[0]
