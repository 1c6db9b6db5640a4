"""GPU decoding of LZW landcover tiles (GCN10_TILE_LZW tiles of gcn10_gpu_inflate_tiles, gcn10_lzw_decode.hip),
through the C ABI and the status words, against the host reader (tiff_codec.c lzw_decode), PIL's libtiff and the
reference decoder of tests/lzw_model.py; and the gcn10 program end to end on LZW landcover."""
import os
import zlib

import numpy as np
import pytest
from PIL import Image

from gcn10_amd import gpu, host
from tests import tiffutil
from tests.test_cli import BLOCKS, ESA_GT, _check_block, _run, _world
from tests.lzw_model import lzw_decode_ref, pack, width_of as _width

pytestmark = pytest.mark.gpu
GUARD = 16              # zero columns / rows around every tile's window in the destination


@pytest.fixture(scope="module")
def engine():
    with gpu.Engine(0) as e:
        yield e


def codes_of(data, clear_every=None, clear=True):
    """LZW codes of data: a dictionary that stops growing at 4096 entries (no Clear when full), or a Clear
    after every clear_every codes."""
    codes = [256] if clear else []
    table, nxt, w, k = {bytes([i]): i for i in range(256)}, 258, b"", 0
    for b in bytes(data):
        wb = w + bytes([b])
        if wb in table:
            w = wb
            continue
        codes.append(table[w])
        k += 1
        if clear_every and k % clear_every == 0:
            codes.append(256)
            table, nxt = {bytes([i]): i for i in range(256)}, 258
        elif nxt < 4096:
            table[wb] = nxt
            nxt += 1
        w = bytes([b])
    if w:
        codes.append(table[w])
    return codes


def _data(kind, n, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "constant":
        return np.full(n, 80, np.uint8)
    if kind == "iid":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "classes":
        codes = np.array([10, 20, 30, 40, 50, 60, 70, 80, 90, 95, 100], np.uint8)
        runs = rng.geometric(0.05, size=n // 8 + 16)
        return np.repeat(codes[rng.integers(0, len(codes), len(runs))], runs)[:n].copy()
    if kind == "patches":
        w = 256
        small = rng.integers(0, 11, ((-(-n // w) + 31) // 32, w // 32), dtype=np.uint8) * 10
        return np.kron(small, np.ones((32, 32), np.uint8)).reshape(-1)[:n].copy()
    raise ValueError(kind)


def run_tiles(engine, streams, out_lens, flags=None, chunk_w=None):
    """Every stream one chunk of out_lens[i] bytes (rows of chunk_w), placed whole in its own band of the
    destination with GUARD zero pixels around it; returns (chunks, status)."""
    n = len(streams)
    flags = flags if flags is not None else [gpu.TILE_LZW] * n
    cw = chunk_w or max(max(out_lens), 1)
    rows = [max(-(-L // cw), 1) for L in out_lens]
    W = cw + 2 * GUARD
    ys, y = [], GUARD
    for r in rows:
        ys.append(y)
        y += r + GUARD
    wins = [(0, 0, cw, out_lens[i] // cw, GUARD, ys[i]) for i in range(n)]
    out, status = engine.inflate_tiles(streams, cw, rows, wins, (y, W), flags=flags,
                                       out_lens=[cw * r if not (f & gpu.TILE_RAW) else L
                                                 for r, f, L in zip(rows, flags, out_lens)])
    guard = out.copy()
    chunks = []
    for i in range(n):
        h = out_lens[i] // cw
        chunks.append(out[ys[i]:ys[i] + h, GUARD:GUARD + cw].reshape(-1).copy())
        guard[ys[i]:ys[i] + h, GUARD:GUARD + cw] = 0
    assert not guard.any(), "bytes written outside the tiles' windows"
    return chunks, status


def _want(stream, n):
    return np.frombuffer(lzw_decode_ref(stream, n), np.uint8)


@pytest.mark.parametrize("kind", ["constant", "iid", "classes", "patches"])
@pytest.mark.parametrize("n", [65536, 4096, 1000, 1])
def test_streams_of_every_kind_decode_as_the_host_does(engine, kind, n):
    data = _data(kind, n, seed=n)
    streams = [tiffutil.lzw_encode(data.tobytes()), pack(codes_of(data) + [257]),
               pack(codes_of(data, clear_every=700) + [257]), pack(codes_of(data, clear_every=37, clear=False) + [257])]
    chunks, status = run_tiles(engine, streams, [n] * 4, chunk_w=256 if n % 256 == 0 else n)
    assert not status.any(), status
    for c in chunks:
        assert np.array_equal(c, data)


def test_dictionary_full_goes_on_at_12_bits_without_a_clear(engine):
    data = _data("iid", 65536, seed=3)
    codes = codes_of(data) + [257]
    assert len(codes) > 20000 and 256 not in codes[1:]      # thousands of codes after the dictionary filled
    stream = pack(codes)
    assert np.array_equal(_want(stream, 65536), data)
    chunks, status = run_tiles(engine, [stream], [65536], chunk_w=256)
    assert status[0] == 0 and np.array_equal(chunks[0], data)


def test_early_eoi_missing_eoi_and_trailing_codes(engine):
    data = _data("classes", 8192, seed=5)
    full = codes_of(data)
    bad = (1 << _width(len(full) - 1)) - 1                      # > next, at the width of the code after them
    streams = [pack(codes_of(data[:3000]) + [257]),            # early EOI: zeros after 3000 bytes
               pack(codes_of(data[:3000])),                     # no EOI, short: an error
               pack(full),                                      # no EOI, exactly full: fine
               pack(codes_of(np.concatenate([data, np.full(500, data[-1], np.uint8)])) + [257]),   # the last code
                                                                # is cut by out_len, codes past it: ignored
               pack(full + [bad, bad, 300]),                    # invalid codes past out_len: ignored
               pack(full + [256, 1, 2, 3, 257])]                # a Clear and codes past out_len: ignored
    last = lzw_decode_ref(streams[3], 8192, trace=True)[1].codes[-1]
    assert last.cut and last.pos + last.length > 8192 + 8
    chunks, status = run_tiles(engine, streams, [8192] * 6, chunk_w=256)
    assert list(status) == [0, gpu.INFLATE_E_LZW_INPUT, 0, 0, 0, 0]
    assert np.array_equal(chunks[0][:3000], data[:3000]) and not chunks[0][3000:].any()
    assert np.array_equal(chunks[0], _want(streams[0], 8192))
    for i in (2, 3, 4, 5):
        assert np.array_equal(chunks[i], data), i
    with pytest.raises(ValueError):
        lzw_decode_ref(streams[1], 8192)


def test_every_error_has_its_status_and_leaves_its_neighbours_alone(engine):
    good = _data("patches", 4096, seed=9)
    gs = tiffutil.lzw_encode(good.tobytes())
    bad = [(pack([256, 65, 300, 257]), gpu.INFLATE_E_LZW_CODE),            # code > next
           (pack([256, 65, 66, 67, 262, 257]), gpu.INFLATE_E_LZW_CODE),
           (pack([258, 257]), gpu.INFLATE_E_LZW_FIRST),                    # first code of the stream
           (pack([256, 300, 257]), gpu.INFLATE_E_LZW_FIRST),               # first code after a Clear
           (pack([256, 65, 66, 256, 259, 257]), gpu.INFLATE_E_LZW_FIRST),  # ... a Clear mid-stream
           (pack([256, 65, 66, 67]), gpu.INFLATE_E_LZW_INPUT),             # no EOI, short
           (b"", gpu.INFLATE_E_LZW_INPUT)]
    streams, want = [], []
    for s, e in bad:
        streams += [gs, s]
        want += [0, e]
        with pytest.raises(ValueError):
            lzw_decode_ref(s, 4096)
    streams.append(gs)
    want.append(0)
    chunks, status = run_tiles(engine, streams, [4096] * len(streams), chunk_w=256)
    assert list(status) == want
    for i in range(0, len(streams), 2):
        assert np.array_equal(chunks[i], good), i
    # LZW may not be combined with RAW
    chunks, status = run_tiles(engine, [gs, gs], [4096, 4096], flags=[gpu.TILE_LZW, gpu.TILE_LZW | gpu.TILE_RAW],
                               chunk_w=256)
    assert list(status) == [0, 1] and np.array_equal(chunks[0], good) and not chunks[1].any()


def test_one_call_mixes_deflate_raw_and_lzw_tiles_with_predictor2(engine):
    datas = [_data(k, 8192, seed=s) for s, k in enumerate(["patches", "iid", "classes", "constant", "patches", "classes"])]

    def diff(a):
        t = a.reshape(-1, 256).astype(np.int16)
        t[:, 1:] -= t[:, :-1].copy()
        return (t & 0xFF).astype(np.uint8).reshape(-1)
    streams = [zlib.compress(datas[0].tobytes()), tiffutil.lzw_encode(datas[1].tobytes()), datas[2].tobytes(),
               tiffutil.lzw_encode(diff(datas[3]).tobytes()), zlib.compress(diff(datas[4]).tobytes()),
               tiffutil.lzw_encode(datas[5].tobytes())]
    flags = [0, gpu.TILE_LZW, gpu.TILE_RAW, gpu.TILE_LZW | gpu.TILE_PREDICTOR2, gpu.TILE_PREDICTOR2, gpu.TILE_LZW]
    chunks, status = run_tiles(engine, streams, [8192] * 6, flags=flags, chunk_w=256)
    assert not status.any(), status
    for i in range(6):
        assert np.array_equal(chunks[i], datas[i]), i
    assert gpu.Engine.inflate_codecs() & gpu.CODEC_LZW


@pytest.mark.parametrize("src,predictor", [("libtiff", 1), ("tiffutil", 1), ("tiffutil", 2)])
@pytest.mark.parametrize("kind", ["patches", "iid", "classes", "constant"])
def test_file_chunks_through_the_plan_equal_host_reader_and_pil(tmp_path, engine, src, kind, predictor):
    """LZW strips written by libtiff (through PIL), LZW tiles written by tests/tiffutil."""
    img = _data(kind, 300 * 520, seed=11).reshape(300, 520)
    p = str(tmp_path / "t.tif")
    if src == "libtiff":
        Image.fromarray(img).save(p, compression="tiff_lzw")
    else:
        tiffutil.write_tiff(p, img, compression=5, tile=(256, 256), predictor=predictor)
    with Image.open(p) as im:
        assert im.tag_v2[259] == 5 and (predictor == 1 or im.tag_v2.get(317) == 2)
        pil = np.array(im)
    with host.Raster(p) as r:
        for (x, y, w, h) in [(0, 0, 520, 300), (100, 37, 300, 200), (255, 255, 2, 2)]:
            plan = r.plan(x, y, w, h, lzw=True)
            chunks = plan[0]
            assert all(c["flags"] & gpu.TILE_LZW for c in chunks)
            got, status = engine.inflate_tiles([c["data"] for c in chunks], chunks[0]["chunk_w"],
                                               [c["rows"] for c in chunks],
                                               [(c["src_x"], c["src_y"], c["copy_w"], c["copy_h"], c["dst_x"],
                                                 c["dst_y"]) for c in chunks], (h, w),
                                               flags=[c["flags"] for c in chunks])
            assert not status.any()
            assert np.array_equal(got, r.read(x, y, w, h)) and np.array_equal(got, pil[y:y + h, x:x + w])


# ---- the program end to end ----------------------------------------------------------------------------------

def _windows_line(log):
    line = [ln for ln in log.splitlines() if "timing: landcover windows:" in ln]
    assert len(line) == 1, line
    return line[0]


def _outputs(tmp_path):
    """Every output raster: its pixels and its tags other than where the tiles lie.  (Not the bytes: the
    writer lays tiles out in the order they are finished, so two runs of the same route already differ there.)"""
    out = {}
    for d in ("cn_rasters_drained", "cn_rasters_undrained"):
        for f in sorted(os.listdir(tmp_path / d)):
            with Image.open(str(tmp_path / d / f)) as im:
                tags = {k: v for k, v in im.tag_v2.items() if k not in (324, 325)}
                out[(d, f)] = (np.array(im), tags)
    return out


@pytest.mark.parametrize("layout", ["tiles", "strips", "predictor2-tiles", "vrt"])
@pytest.mark.parametrize("prefetch", [1, 0], ids=["one-block-ahead", "in-turn"])
def test_lzw_landcover_through_the_gpu_decoder_and_the_host_reader(tmp_path, tables, layout, prefetch):
    runs = {}
    for lzw_on in (1, 0):
        d = tmp_path / ("gpu" if lzw_on else "host")
        d.mkdir()
        esa, soil = _world(d, seed=83, extra_cfg="prefetch_blocks=%d\ngpu_inflate_lzw=%d\n" % (prefetch, lzw_on))
        if layout == "vrt":
            # DEFLATE tiles west of x = 1500, LZW tiles east of it: blocks 101 and 102 cross the seam
            tiffutil.write_tiff(str(d / "w.tif"), esa[:, :1500], compression=8, tile=(256, 256))
            tiffutil.write_tiff(str(d / "e.tif"), esa[:, 1500:], compression=5, tile=(256, 256), predictor=2)
            src = "".join('<SimpleSource><SourceFilename relativeToVRT="1">%s</SourceFilename><SourceBand>1</SourceBand>'
                          '<SrcRect xOff="0" yOff="0" xSize="%d" ySize="2000" /><DstRect xOff="%d" yOff="0" xSize="%d" '
                          'ySize="2000" /></SimpleSource>\n' % (n, w, x, w) for n, x, w in (("w.tif", 0, 1500),
                                                                                           ("e.tif", 1500, 1500)))
            (d / "esa.vrt").write_text(
                '<VRTDataset rasterXSize="3000" rasterYSize="2000">\n<GeoTransform> %r, %r, 0.0, %r, 0.0, %r'
                '</GeoTransform>\n<VRTRasterBand dataType="Byte" band="1">\n%s</VRTRasterBand></VRTDataset>\n'
                % (ESA_GT[0], ESA_GT[1], ESA_GT[3], ESA_GT[5], src))
            cfg = (d / "config.txt").read_text().replace(str(d / "esa.tif"), str(d / "esa.vrt"))
            (d / "config.txt").write_text(cfg)
        else:
            kw = {"tiles": dict(tile=(512, 512)), "strips": dict(rows_per_strip=37),
                  "predictor2-tiles": dict(tile=(256, 256), predictor=2)}[layout]
            tiffutil.write_tiff(str(d / "esa.tif"), esa, gt=ESA_GT, compression=5, **kw)
        (d / "ids.txt").write_text("101 102 103\n")
        out = _run(d, "-c", "config.txt", "-l", "ids.txt")
        assert out.returncode == 0, out.stderr[-2000:]
        # (the VRT: block 101 lies west of the seam, all DEFLATE: through the GPU decoder on both routes)
        want = {(1, False): (3, 3, 0), (0, False): (0, 0, 3), (1, True): (3, 2, 0), (0, True): (1, 0, 2)}
        line = _windows_line((d / "logs" / "rank_0.log").read_text())
        assert line.endswith("landcover windows: %d through the gpu decoder (of them %d with lzw chunks), "
                             "%d through the host reader" % want[lzw_on, layout == "vrt"]), line
        for bid, *bbox in BLOCKS[:3]:
            _check_block(d, esa, soil, tables, bid, bbox)
        runs[lzw_on] = _outputs(d)
    assert runs[0].keys() == runs[1].keys() and len(runs[0]) == 54
    for k in runs[0]:
        assert np.array_equal(runs[0][k][0], runs[1][k][0]) and runs[0][k][1] == runs[1][k][1], k


def test_corrupt_lzw_tile_fails_its_block_on_both_routes(tmp_path, tables):
    for lzw_on in (1, 0):
        d = tmp_path / ("gpu" if lzw_on else "host")
        d.mkdir()
        esa, soil = _world(d, seed=84, extra_cfg="gpu_inflate_lzw=%d\n" % lzw_on)
        path = d / "esa.tif"
        tiffutil.write_tiff(str(path), esa, gt=ESA_GT, compression=5, tile=(512, 512))
        raw = bytearray(path.read_bytes())
        im = Image.open(str(path))
        offs, cnts = im.tag_v2[324], im.tag_v2[325]
        k = 2 * ((3000 + 511) // 512) + 3                    # tile (row 2, col 3): block 102 only
        for i in range(offs[k] + 2, offs[k] + cnts[k]):
            raw[i] = 0xFF
        path.write_bytes(bytes(raw))
        (d / "ids.txt").write_text("101 102\n")
        out = _run(d, "-c", "config.txt", "-l", "ids.txt")
        assert out.returncode == 0, out.stderr[-2000:]
        log = (d / "logs" / "rank_0.log").read_text()
        assert "gdalrasterio error: cannot decode a tile of the window" in log
        assert "[ERROR] [rank 0] esa load failed for block 102" in log
        assert not (d / "cn_rasters_drained" / "cn_p_i_102.tif").exists()
        _check_block(d, esa, soil, tables, 101, BLOCKS[0][1:])
        assert ("through the gpu decoder (of them 2 with lzw chunks)" if lzw_on else "2 through the host reader") \
            in _windows_line(log)
