"""Read plans of LZW landcover for the GPU decoder (host/raster.c, tiff_window.c: gcn10_raster_plan_window_codecs),
and the config key gpu_inflate_lzw.  No GPU needed: the plans are carried out here with a Python LZW decoder
and numpy, and compared with the host reader."""
import numpy as np
import pytest

from gcn10_amd import host
from tests import tiffutil
from tests.lzw_model import lzw_decode_ref  # noqa: F401  (its old home: other tests import it from here)

TILE_RAW, TILE_PREDICTOR2, TILE_LZW = 1, 2, 4
GT = [-111.0, 0.01, 0.0, 39.0, 0.0, -0.02]


def _img(seed, H, W):
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 12, size=((H + 7) // 8, (W + 7) // 8), dtype=np.uint8) * 10
    img = np.repeat(np.repeat(small, 8, axis=0), 8, axis=1)[:H, :W].copy()
    noise = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    return np.where(noise < 40, noise, img).astype(np.uint8)


def _assemble(plan, W, H):
    """What gcn10_gpu_inflate_tiles does with a plan, done with lzw_decode_ref, zlib and numpy."""
    import zlib
    chunks, covered, max_bytes = plan
    out = np.zeros((H, W), np.uint8)
    seen = 0
    for c in chunks:
        cw = c["chunk_w"]
        assert not (c["flags"] & TILE_RAW and c["flags"] & TILE_LZW)
        if c["flags"] & TILE_RAW:
            raw = np.frombuffer(c["data"], np.uint8)
            t = np.zeros(-(-raw.size // cw) * cw, np.uint8)
            t[:raw.size] = raw
        else:
            assert c["out_len"] == cw * c["rows"] and c["out_len"] <= max_bytes
            if c["flags"] & TILE_LZW:
                t = np.frombuffer(lzw_decode_ref(c["data"], c["out_len"]), np.uint8).copy()
            else:
                t = np.frombuffer(zlib.decompress(c["data"]), np.uint8)[:c["out_len"]].copy()
        t = t.reshape(-1, cw)
        if c["flags"] & TILE_PREDICTOR2:
            t = np.cumsum(t, axis=1, dtype=np.uint64).astype(np.uint8)
        out[c["dst_y"]:c["dst_y"] + c["copy_h"], c["dst_x"]:c["dst_x"] + c["copy_w"]] = \
            t[c["src_y"]:c["src_y"] + c["copy_h"], c["src_x"]:c["src_x"] + c["copy_w"]]
        seen += c["copy_w"] * c["copy_h"]
    assert seen == covered
    return out


WINDOWS = [(0, 0, 101, 75), (13, 9, 50, 41), (100, 74, 1, 1), (31, 15, 2, 2), (0, 70, 101, 5), (64, 0, 37, 75)]


@pytest.mark.parametrize("kw", [dict(tile=(32, 16)), dict(tile=(64, 64)), dict(rows_per_strip=7), dict(),
                                dict(tile=(16, 16), bigtiff=True), dict(rows_per_strip=3, big_endian=True),
                                dict(tile=(32, 32), predictor=2), dict(rows_per_strip=11, predictor=2),
                                dict(tile=(16, 16), predictor=2, bigtiff=True, big_endian=True)], ids=str)
def test_lzw_plan_reassembles_every_window(tmp_path, kw):
    img = _img(21, 75, 101)
    p = str(tmp_path / "t.tif")
    tiffutil.write_tiff(p, img, gt=GT, compression=5, **kw)
    want_flags = TILE_LZW | (TILE_PREDICTOR2 if kw.get("predictor") == 2 else 0)
    with host.Raster(p) as r:
        for (x, y, w, h) in WINDOWS:
            plan = r.plan(x, y, w, h, lzw=True)
            assert plan is not None and plan[1] == w * h
            assert {c["flags"] for c in plan[0]} == {want_flags}
            got = _assemble(plan, w, h)
            assert np.array_equal(got, img[y:y + h, x:x + w]), (x, y, w, h)
            assert np.array_equal(got, r.read(x, y, w, h))
            # the plan without the codec mask still declines (gcn10_raster_plan_window's contract)
            assert r.plan(x, y, w, h) is None
        with pytest.raises(host.HostError):
            r.plan(90, 0, 20, 5, lzw=True)


@pytest.mark.parametrize("kw", [dict(compression=8, tile=(32, 32)), dict(compression=1, rows_per_strip=7),
                                dict(compression=8, predictor=2, rows_per_strip=5)], ids=str)
def test_lzw_mask_plans_other_codecs_as_before(tmp_path, kw):
    img = _img(22, 40, 60)
    p = str(tmp_path / "t.tif")
    tiffutil.write_tiff(p, img, gt=GT, **kw)
    with host.Raster(p) as r:
        for win in [(0, 0, 60, 40), (7, 3, 30, 20)]:
            a, b = r.plan(*win), r.plan(*win, lzw=True)
            assert a is not None and b is not None
            assert [dict(c) for c in a[0]] == [dict(c) for c in b[0]] and a[1:] == b[1:]


def test_lzw_mask_still_declines_packbits(tmp_path):
    p = str(tmp_path / "t.tif")
    tiffutil.write_tiff(p, _img(8, 40, 60), gt=GT, compression=32773, rows_per_strip=9)
    with host.Raster(p) as r:
        assert r.plan(0, 0, 60, 40, lzw=True) is None


def _mixed_vrt(tmp_path, pred_b=1):
    """Two sources side by side with a seam at x = 64: DEFLATE tiles left, LZW tiles right."""
    a, b = _img(31, 64, 64), _img(32, 64, 70)
    tiffutil.write_tiff(str(tmp_path / "a.tif"), a, compression=8, tile=(32, 32))
    tiffutil.write_tiff(str(tmp_path / "b.tif"), b, compression=5, tile=(16, 16), predictor=pred_b)
    src = """    <SimpleSource>
      <SourceFilename relativeToVRT="1">%s</SourceFilename>
      <SourceBand>1</SourceBand>
      <SrcRect xOff="0" yOff="0" xSize="%d" ySize="64" />
      <DstRect xOff="%d" yOff="4" xSize="%d" ySize="64" />
    </SimpleSource>
"""
    vrt = ("""<VRTDataset rasterXSize="140" rasterYSize="72">
  <GeoTransform> -1.8000000000000000e+02,  8.3333333333330430e-05,  0.0000000000000000e+00,  8.4000000000000000e+01,  0.0000000000000000e+00, -8.3333333333330430e-05</GeoTransform>
  <VRTRasterBand dataType="Byte" band="1">
""" + src % ("a.tif", 64, 0, 64) + src % ("b.tif", 70, 64, 70) + """  </VRTRasterBand>
</VRTDataset>
""")
    (tmp_path / "m.vrt").write_text(vrt)
    exp = np.zeros((72, 140), np.uint8)
    exp[4:68, :64] = a
    exp[4:68, 64:134] = b
    return exp


@pytest.mark.parametrize("pred_b", [1, 2])
def test_lzw_plan_of_a_vrt_mixing_lzw_and_deflate_sources(tmp_path, pred_b):
    exp = _mixed_vrt(tmp_path, pred_b)
    with host.Raster(str(tmp_path / "m.vrt")) as r:
        assert np.array_equal(r.read(0, 0, 140, 72), exp)
        for (x, y, w, h) in [(0, 0, 140, 72), (50, 10, 30, 30), (60, 0, 8, 72), (100, 30, 40, 42)]:
            plan = r.plan(x, y, w, h, lzw=True)
            assert plan is not None
            flags = {c["flags"] for c in plan[0]}
            if x < 64 < x + w:
                assert flags == {0, TILE_LZW | (TILE_PREDICTOR2 if pred_b == 2 else 0)}
            assert np.array_equal(_assemble(plan, w, h), exp[y:y + h, x:x + w]), (x, y, w, h)
            assert r.plan(x, y, w, h) is None if x + w > 64 else r.plan(x, y, w, h) is not None


def test_python_lzw_decoder_matches_the_host_reader_on_edge_streams(tmp_path):
    """The reference decoder of these tests against the host reader, on a stream with an early EOI:
    both leave zeros after it."""
    img = np.random.default_rng(5).integers(0, 256, size=(8, 16), dtype=np.uint8)
    p = str(tmp_path / "t.tif")
    tiffutil.write_tiff(p, img, gt=GT, compression=5, tile=(16, 16))
    with host.Raster(p) as r:
        chunk = r.plan(0, 0, 16, 8, lzw=True)[0][0]
    short = tiffutil.lzw_encode(bytes(range(40)))           # 40 bytes, then EOI: the tile holds 256
    data = bytearray(open(p, "rb").read())
    off = bytes(data).find(chunk["data"])
    assert off > 0 and len(short) <= len(chunk["data"])
    data[off:off + len(short)] = short
    open(p, "wb").write(bytes(data))
    with host.Raster(p) as r:
        got = r.read(0, 0, 16, 8)
    want = np.frombuffer(lzw_decode_ref(short, 256), np.uint8).reshape(16, 16)[:8]
    assert np.array_equal(got, want) and not got.reshape(-1)[40:].any()


def test_gpu_inflate_lzw_config_key(tmp_path):
    base = "hysogs_data_path=a\nesa_data_path=b\nblocks_shp_path=c\nlookup_table_path=d\nlog_dir=e\n"
    p = tmp_path / "c.txt"
    p.write_text(base)
    assert host.parse_config(str(p))["gpu_inflate_lzw"] == 1
    p.write_text(base + "gpu_inflate_lzw=0\n")
    c = host.parse_config(str(p))
    assert c["gpu_inflate_lzw"] == 0 and c["gpu_inflate"] == 1
    p.write_text(base + "gpu_inflate_lzw=1\ngpu_inflate=0\n")
    c = host.parse_config(str(p))
    assert c["gpu_inflate_lzw"] == 1 and c["gpu_inflate"] == 0
