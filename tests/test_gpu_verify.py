"""GPU: the raster verifier (gcn10_gpu_verify_strip / gcn10_gpu_verify_buffers) against the oracle.  The oracle's 18
rasters of a block are uploaded as the "file" rasters: unchanged they must give no mismatch, with pixels changed at
known places the counters must name exactly those, whatever the strips the block is cut into.  Every comparison is
exact."""
import numpy as np
import pytest

from gcn10_amd import gpu, host
from oracle import cn_oracle_c as oc
from tests.util import make_block, random_tables

pytestmark = pytest.mark.gpu

NONE = gpu.VERIFY_NONE
# (H, W, soil rows, soil columns)
SHAPES = [(300, 1040, 12, 42), (97, 1000, 9, 33), (64, 1037, 7, 40), (1, 555, 3, 20), (5, 17, 2, 3), (33, 16, 4, 2),
          (70, 36001, 5, 700), (36001, 70, 700, 5)]


def strips_of(H, cuts):
    """[(y0, rows)] of a block cut at the given rows"""
    edges = [0] + [c for c in cuts if 0 < c < H] + [H]
    return [(a, b - a) for a, b in zip(edges[:-1], edges[1:])]


class Block:
    """One block on the device: landcover, soil and index maps, the tile prepared."""

    def __init__(self, eng, tables, shape, seed, nasty=True):
        H, W, hsy, hsx = shape
        self.eng, self.H, self.W = eng, H, W
        self.esa, gt, coarse, sgt = make_block(seed, H, W, hsy, hsx, nasty=nasty)
        self.want = oc.process_block_mem(self.esa, gt, coarse, sgt, tables)      # [18, H, W]: the oracle
        ci, cj = host.build_index_maps(gt, sgt, W, H, hsx, hsy)
        eng.set_tables(tables)
        self.bufs = [eng.upload(a) for a in (self.esa, coarse, ci, cj)]
        eng.prepare_tile(self.bufs[1].ptr, hsx, hsy, self.bufs[2].ptr, W)

    def close(self):
        for b in self.bufs:
            b.close()

    def verify(self, got, strips, cond_mask=3, table_mask=0x1FF, pad=0, seed=0, preset=None):
        """got: uint8[18, H, W] "file" rasters.  Uploaded with rows `W + pad` bytes apart (the padding holds noise),
        verified strip by strip.  Returns the counters and checks that the buffers were not written to."""
        eng, H, W = self.eng, self.H, self.W
        stride = W + pad
        host_got = np.random.default_rng(seed).integers(0, 256, size=(18, H, stride), dtype=np.uint8)
        host_got[:, :, :W] = got
        dev = eng.upload(host_got)
        counts = eng.verify_counts_alloc()
        if preset is not None:
            eng.h2d(counts.ptr, preset)
            eng.sync()
        try:
            for y0, rows in strips:
                ptrs = [dev.ptr + (r * H + y0) * stride for r in range(18)]
                eng.verify_strip(self.bufs[0].ptr + y0 * W, W, rows, self.bufs[3].ptr + 4 * y0, cond_mask, table_mask,
                                 ptrs, stride, y0, counts.ptr)
            out = eng.verify_counts(counts.ptr)
            after = eng.download(dev.ptr, host_got.shape)
        finally:
            dev.close()
            counts.close()
        assert np.array_equal(after, host_got), "the verifier wrote to the file rasters"
        return out


def selected(cond_mask, table_mask):
    return [r for r in range(18) if (cond_mask >> (r // 9)) & 1 and (table_mask >> (r % 9)) & 1]


def cuts_for(H):
    return [[], [H // 3], [1, H // 2, H // 2 + 1, H - 1], list(range(7, H, 29))[:40]]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % (s[1], s[0]))
@pytest.mark.parametrize("which", ["shipped", "random"])
def test_oracle_rasters_verify_clean(engine, tables, shape, which):
    blk = Block(engine, tables if which == "shipped" else random_tables(shape[0] + shape[1]), shape, seed=shape[1])
    try:
        for i, cuts in enumerate(cuts_for(blk.H)):
            pad = (0, 23, 256, 1)[i]
            out = blk.verify(blk.want, strips_of(blk.H, cuts), pad=pad, seed=i)
            print("clean %s %s strips=%d pad=%d mismatches=%s" % (shape, which, len(strips_of(blk.H, cuts)), pad,
                                                                  out["mismatches"].tolist()))
            assert out["mismatches"].tolist() == [0] * 18
            assert out["first"].tolist() == [NONE] * 18
    finally:
        blk.close()


@pytest.mark.parametrize("cond_mask,table_mask", [(1, 0x1FF), (2, 1 << 7), (3, 0x0A1), (2, 0x111)])
def test_subset_of_rasters_leaves_the_others_alone(engine, tables, cond_mask, table_mask):
    blk = Block(engine, tables, SHAPES[2], seed=5)
    try:
        sel = selected(cond_mask, table_mask)
        # garbage in every raster that is not selected, and markers in their counters
        got = blk.want.copy()
        for r in range(18):
            if r not in sel:
                got[r] ^= 0x5A
        preset = np.zeros(18, gpu.VERIFY_COUNT_DTYPE)
        preset["first"] = NONE
        for r in range(18):
            if r not in sel:
                preset[r] = (1000 + r, 77 + r, 3, 4)
        out = blk.verify(got, strips_of(blk.H, [10, 40]), cond_mask, table_mask, pad=5, preset=preset)
        for r in range(18):
            if r in sel:
                assert (out[r]["mismatches"], out[r]["first"]) == (0, NONE), r
            else:
                assert out[r].tolist() == preset[r].tolist(), r
        # and one planted pixel per selected raster is found with the subset's kernel too
        y, x = blk.H - 1, blk.W - 1
        for r in sel:
            got[r, y, x] ^= 0x80
        out = blk.verify(got, strips_of(blk.H, [10, 40]), cond_mask, table_mask, pad=5, preset=preset)
        for r in sel:
            assert out[r].tolist() == (1, (y << 32) | x, int(blk.want[r, y, x]), int(got[r, y, x])), r
    finally:
        blk.close()


def plant(want, places):
    """places: {raster: [(y, x), ...]} -> the rasters with those pixels changed, and the expected counters"""
    got = want.copy()
    exp = np.zeros(18, gpu.VERIFY_COUNT_DTYPE)
    exp["first"] = NONE
    for r, pts in places.items():
        for k, (y, x) in enumerate(sorted(set(pts))):
            got[r, y, x] = (int(want[r, y, x]) + 1 + k % 255) % 256    # never the value itself
            assert got[r, y, x] != want[r, y, x]
        y, x = min(set(pts))
        exp[r] = (len(set(pts)), (y << 32) | x, int(want[r, y, x]), int(got[r, y, x]))
    return got, exp


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % (s[1], s[0]))
def test_planted_pixels_are_counted_and_located(engine, tables, shape):
    blk = Block(engine, tables, shape, seed=11, nasty=False)
    try:
        H, W = blk.H, blk.W
        rng = np.random.default_rng(H * 7 + W)
        rand = lambda n: [(int(rng.integers(0, H)), int(rng.integers(0, W))) for _ in range(n)]
        places = {
            0: [(0, 0)],                                        # first pixel
            4: [(H - 1, W - 1)],                                # last pixel (in the W % 16 tail where there is one)
            7: [(0, 0), (H - 1, W - 1)] + rand(40),
            9: rand(5) + [(H // 2, min(W - 1, 15)), (H // 2, min(W - 1, 16))],
            13: [(H - 1, 0)],
            17: rand(300),
        }
        # a pixel whose computed value is 255, in a raster of its own
        nodata = np.argwhere(blk.want[2] == 255)
        assert len(nodata) or H * W < 10000, "the block has no 255 in raster 2"
        if len(nodata):
            places[2] = [tuple(int(v) for v in nodata[len(nodata) // 2])]
        got, exp = plant(blk.want, places)
        assert 2 not in places or exp[2]["want"] == 255
        outs = []
        for i, cuts in enumerate(cuts_for(H)):
            out = blk.verify(got, strips_of(H, cuts), pad=(0, 9, 48, 3)[i], seed=i)
            print("planted %s strips=%d: %s" % (shape, len(strips_of(H, cuts)), out.tolist()))
            outs.append(out)
        for out in outs:
            for r in range(18):
                assert out[r].tolist()[:2] == exp[r].tolist()[:2], r
                if r in places:
                    assert out[r].tolist() == exp[r].tolist(), r
            assert np.array_equal(out, outs[0])                  # one strip or many: the same counters
    finally:
        blk.close()


def test_every_pixel_wrong(engine, tables):
    """A raster of another table in a file's place: every differing pixel is counted (no 32-bit or per-wave cap)."""
    blk = Block(engine, tables, (513, 2000, 20, 70), seed=3, nasty=False)
    try:
        got = blk.want.copy()
        got[5] = blk.want[8]
        got[12] = 255 - blk.want[12]
        out = blk.verify(got, strips_of(blk.H, [256]), pad=16)
        for r, n in ((5, int((blk.want[5] != blk.want[8]).sum())), (12, blk.H * blk.W)):
            ys, xs = np.nonzero(got[r] != blk.want[r])
            assert out[r].tolist() == (n, (int(ys[0]) << 32) | int(xs[0]), int(blk.want[r, ys[0], xs[0]]),
                                       int(got[r, ys[0], xs[0]])), r
        assert sum(int(out[r]["mismatches"]) for r in range(18) if r not in (5, 12)) == 0
    finally:
        blk.close()


@pytest.mark.parametrize("H,W", [(300, 1040), (41, 1003), (1, 17), (9, 5), (70, 36001)])
def test_verify_buffers(engine, tables, H, W):
    rng = np.random.default_rng(H + W)
    want = rng.integers(0, 256, size=(18, H, W), dtype=np.uint8)
    mask = 0x3FFFF if W % 2 else 0x2A5A5
    places = {0: [(0, 0)], 2: [(H - 1, W - 1)], 5: [(H // 2, W // 2), (H - 1, 0), (0, W - 1)],
              17: [(int(rng.integers(0, H)), int(rng.integers(0, W))) for _ in range(100)]}
    places = {r: p for r, p in places.items() if (mask >> r) & 1}
    got_planted, exp = plant(want, places)
    for got, expect in ((want, None), (got_planted, exp)):
        ws, gs = W + 7, W + 32
        hw = rng.integers(0, 256, size=(18, H, ws), dtype=np.uint8)
        hg = rng.integers(0, 256, size=(18, H, gs), dtype=np.uint8)
        hw[:, :, :W] = want
        hg[:, :, :W] = got
        dw, dg = engine.upload(hw), engine.upload(hg)
        results = []
        try:
            for cuts in ([], [H // 2], list(range(1, H, 13))):
                counts = engine.verify_counts_alloc()
                for y0, rows in strips_of(H, cuts):
                    engine.verify_buffers([dw.ptr + (r * H + y0) * ws for r in range(18)], ws,
                                          [dg.ptr + (r * H + y0) * gs for r in range(18)], gs, W, rows, y0, mask,
                                          counts.ptr)
                results.append(engine.verify_counts(counts.ptr))
                counts.close()
            assert np.array_equal(engine.download(dg.ptr, hg.shape), hg)
            assert np.array_equal(engine.download(dw.ptr, hw.shape), hw)
        finally:
            dw.close()
            dg.close()
        for out in results:
            print("buffers %dx%d planted=%s: %s" % (W, H, expect is not None, out["mismatches"].tolist()))
            if expect is None:
                assert out["mismatches"].tolist() == [0] * 18 and out["first"].tolist() == [NONE] * 18
            else:
                assert out.tolist() == expect.tolist()
            assert np.array_equal(out, results[0])


def test_bad_arguments_are_refused(engine, tables):
    blk = Block(engine, tables, SHAPES[0], seed=1)
    counts = engine.verify_counts_alloc()
    try:
        ptrs = [blk.bufs[0].ptr] * 18
        with pytest.raises(gpu.Gcn10GpuError):          # rows closer together than the raster is wide
            engine.verify_strip(blk.bufs[0].ptr, blk.W, 4, blk.bufs[3].ptr, 3, 0x1FF, ptrs, blk.W - 1, 0, counts.ptr)
        with pytest.raises(gpu.Gcn10GpuError):          # another width than the prepared tile's
            engine.verify_strip(blk.bufs[0].ptr, blk.W - 16, 4, blk.bufs[3].ptr, 3, 0x1FF, ptrs, blk.W, 0, counts.ptr)
        with pytest.raises(gpu.Gcn10GpuError):          # a selected raster without a pointer
            engine.verify_strip(blk.bufs[0].ptr, blk.W, 4, blk.bufs[3].ptr, 3, 0x1FF, ptrs[:17] + [None], blk.W, 0,
                                counts.ptr)
        with pytest.raises(gpu.Gcn10GpuError):
            engine.verify_buffers(ptrs, blk.W, ptrs, blk.W, blk.W, 4, 0, 1 << 18, counts.ptr)
    finally:
        counts.close()
        blk.close()
