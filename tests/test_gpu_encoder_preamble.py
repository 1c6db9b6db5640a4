"""GPU: what the three tile encoders answer BEFORE they launch anything -- the shape, pointer, arena and offset
checks of the arena / table / cursor contract they share -- that a refused call leaves the context fit for the
next good one, and that a good one lays its streams out as the contract says.  Needs an MI355X.

The entry points: gcn10_gpu_deflate_strip, gcn10_gpu_lzw_strip (n rasters held in device memory) and
gcn10_gpu_deflate_fused_strip (landcover + prepared soil, the rasters named by two masks).  One engine for the
module, on it one tile of 257 x 257 pixels: four tile positions, three of them edge tiles.  The two rasters every
encoder is given are the oracle's rasters 0 and 1 of that tile (cond_mask = 1, table_mask = 3 for the fused one).

  refusals   exactly one thing wrong per call, so the order of the checks cannot matter; every bad argument is one
             the library refuses on the host, no memory is touched: zero and 19 rasters (the per-raster encoders),
             W = 0, rows = -1, a null arena, a null table, a null cursor, an arena 8 bytes into its allocation,
             arena_cap = 0xfffffffe beside a small arena.  All are GCN10_E_INVAL but one: the fused encoder takes its
             width from the prepared tile, so W = 0 is "no tile prepared for this width" there, GCN10_E_STATE (as
             tests/test_gpu_reader_preamble.py pins for every width but the prepared one).
             After each refusal the same engine encodes the tile again, byte for byte what it did when checked.
  rows = 0   success with a null arena, table and cursor; a real cursor keeps the sentinel it held.
  valid      every stream decodes (zlib; the strict LZW decoder of tests/test_gpu_lzw.py) to its source tile, a
             raster's streams follow one another in 16-byte slots, its first lies at a multiple of 4 096, and the
             cursor is the end of the last raster's extent.  The corner tile is one pixel, 0 in both rasters: the
             fused encoder emits it once and gives raster 1 the entry of raster 0; the other two encode it twice.
  bounds     gcn10_gpu_deflate_arena_bound as tests/test_gpu_deflate.py::test_argument_errors pins it;
             gcn10_gpu_lzw_arena_bound the same formula with the LZW stream maximum of 82 032 bytes.

The codes and bounds are those of the code before the three job setups were folded into one
(profiles/codec_split/preamble_on_parent.txt: this module run against that library).
"""
import zlib

import numpy as np
import pytest

from gcn10_amd import gpu
from tests import soil_readers as sr
from tests.test_gpu_lzw import strict_lzw_decode

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_STATE = 0, -1, -4
W = H = 257
ACROSS = DOWN = 2
N = 2                               # rasters 0 and 1: cond_mask 1, table_mask 3
COND, TABLES = 1, 3
SENTINEL = 0x5EA15EA15EA15EA1
ENCODERS = ("deflate", "lzw", "fused")
NAMES = {"deflate": "gcn10_gpu_deflate_strip", "lzw": "gcn10_gpu_lzw_strip", "fused": "gcn10_gpu_deflate_fused_strip"}
MAX_STREAM = {"deflate": 65552, "lzw": 82032, "fused": 65552}


class World:
    """The engine, the prepared tile, its two rasters on the device, and every encoder's checked result."""

    def __init__(self, tables):
        self.eng = gpu.Engine(0)
        self.eng.set_tables(tables)
        self.tile = sr.ReaderTile(self.eng, tables, seed=41, W=W, H=H, hsx=9, hsy=9, key="encoder-preamble-257")
        self.tile.prepare()
        self.want = [self.tile.want(r) for r in range(N)]
        self.rasters = [self.eng.upload(r) for r in self.want]
        self.ptrs = self.eng.upload(np.array([b.ptr for b in self.rasters], dtype=np.uint64))
        cap = max(int(gpu.lib().gcn10_gpu_lzw_arena_bound(W, H, N)), int(gpu.lib().gcn10_gpu_deflate_arena_bound(W, H, N)))
        self.arena, self.cap = self.eng.alloc(cap), cap
        self.table = self.eng.alloc(N * ACROSS * DOWN * 8)
        self.cursor = self.eng.alloc(8)
        self.eng.sync()
        self.checked = {}

    def close(self):
        self.eng.sync()
        self.eng.close()

    def call(self, enc, n=N, w=W, rows=H, arena=True, cap=None, table=True, cursor=True):
        """The return code of one call of the entry point on the module's buffers; arena / table / cursor: True = the
        real one, None = null, a number = that address."""
        L, c = gpu.lib(), self.eng._ctx
        real = {"arena": self.arena.ptr, "table": self.table.ptr, "cursor": self.cursor.ptr}
        a, t, u = (real[k] if v is True else v for k, v in (("arena", arena), ("table", table), ("cursor", cursor)))
        cap = self.cap if cap is None else cap
        if enc == "deflate":
            return L.gcn10_gpu_deflate_strip(c, self.ptrs.ptr, n, w, rows, a, cap, t, u, None)
        if enc == "lzw":
            return L.gcn10_gpu_lzw_strip(c, self.ptrs.ptr, n, w, rows, a, cap, t, u, None)
        assert enc == "fused" and n == N
        return L.gcn10_gpu_deflate_fused_strip(c, self.tile.bufs[0].ptr, w, rows, self.tile.bufs[3].ptr, COND, TABLES,
                                               a, cap, t, u, None)

    def encode(self, enc):
        """One good run through the Python face: (arena bytes, table, used)."""
        if enc == "deflate":
            return self.eng.deflate_rasters([b.ptr for b in self.rasters], W, H)
        if enc == "lzw":
            return self.eng.lzw_strip([b.ptr for b in self.rasters], W, H)
        return self.eng.deflate_fused(self.tile.bufs[0].ptr, W, H, self.tile.bufs[3].ptr, COND, TABLES)

    def source_tile(self, r, ty, tx):
        src = np.zeros((256, 256), np.uint8)
        part = self.want[r][ty * 256:(ty + 1) * 256, tx * 256:(tx + 1) * 256]
        src[:part.shape[0], :part.shape[1]] = part
        return src

    def check(self, enc):
        """The good run, every stream decoded and the layout held to the contract; done once per encoder, kept."""
        if enc in self.checked:
            return self.checked[enc]
        data, table, used = self.encode(enc)
        assert table.shape == (N, DOWN, ACROSS, 2)
        end = 0
        for r in range(N):
            assert int(table[r, 0, 0, 0]) % 4096 == 0, "raster %d starts at %d" % (r, int(table[r, 0, 0, 0]))
            assert int(table[r, 0, 0, 0]) >= end
            end = int(table[r, 0, 0, 0])
            for ty in range(DOWN):
                for tx in range(ACROSS):
                    off, size = int(table[r, ty, tx, 0]), int(table[r, ty, tx, 1])
                    assert 0 < size <= MAX_STREAM[enc], (enc, r, ty, tx, size)
                    src = self.source_tile(r, ty, tx)
                    stream = data[off:off + size]
                    got = strict_lzw_decode(stream, 65536)[0] if enc == "lzw" else zlib.decompress(stream.tobytes())
                    assert got == src.tobytes(), (enc, r, ty, tx)
                    # the fused encoder emits one stream where two of its rasters are the same bytes (here the corner
                    # tile, a single pixel that is 0 in both): the later raster's entry is the earlier one's
                    twin = [q for q in range(r) if enc == "fused" and np.array_equal(self.source_tile(q, ty, tx), src)]
                    if twin:
                        assert (off, size) == tuple(int(v) for v in table[twin[0], ty, tx]), (enc, r, ty, tx)
                        continue
                    assert off == end, (enc, r, ty, tx, off, end)
                    end = off + (size + 15) // 16 * 16
        assert used == end, "%s: used = %d, the last extent ends at %d" % (NAMES[enc], used, end)
        self.checked[enc] = (data, table, used)
        return self.checked[enc]

    def good_call(self, enc):
        """The engine still works: the same run gives the checked bytes again."""
        data, table, used = self.check(enc)
        again = self.encode(enc)
        assert again[2] == used and np.array_equal(again[1], table) and np.array_equal(again[0], data), NAMES[enc]


@pytest.fixture(scope="module")
def world(tables):
    w = World(tables)
    try:
        yield w
    finally:
        w.close()


def refused(world, enc, rc, code=E_INVAL):
    """rc as the Python face reports it: Gcn10GpuError with that code, naming the entry point."""
    with pytest.raises(gpu.Gcn10GpuError) as e:
        world.eng._chk(rc, NAMES[enc])
    assert e.value.code == code, str(e.value)
    world.good_call(enc)


@pytest.mark.parametrize("enc", ENCODERS)
def test_a_good_strip_decodes_and_lies_where_the_contract_says(world, enc):
    world.check(enc)


@pytest.mark.parametrize("n", [0, 19])
@pytest.mark.parametrize("enc", ["deflate", "lzw"])
def test_raster_count_out_of_range(world, enc, n):
    refused(world, enc, world.call(enc, n=n))


@pytest.mark.parametrize("enc", ENCODERS)
def test_zero_width(world, enc):
    # (the fused encoder: a width other than the prepared tile's is a missing prepare_tile, not a bad argument)
    refused(world, enc, world.call(enc, w=0), E_STATE if enc == "fused" else E_INVAL)


@pytest.mark.parametrize("enc", ENCODERS)
def test_negative_rows(world, enc):
    refused(world, enc, world.call(enc, rows=-1))


@pytest.mark.parametrize("which", ["arena", "table", "cursor"])
@pytest.mark.parametrize("enc", ENCODERS)
def test_null_pointer(world, enc, which):
    refused(world, enc, world.call(enc, **{which: None}))


@pytest.mark.parametrize("enc", ENCODERS)
def test_arena_not_16_byte_aligned(world, enc):
    refused(world, enc, world.call(enc, arena=world.arena.ptr + 8, cap=world.cap - 8))


@pytest.mark.parametrize("enc", ENCODERS)
def test_arena_cap_beyond_32_bit_offsets(world, enc):
    # straight at the library: the Python face would try to allocate the cap
    refused(world, enc, world.call(enc, cap=0xFFFFFFFE))


@pytest.mark.parametrize("enc", ENCODERS)
def test_an_empty_strip_is_success_and_touches_nothing(world, enc):
    assert world.call(enc, rows=0, arena=None, table=None, cursor=None) == OK, gpu.lib().gcn10_gpu_last_error().decode()
    world.eng.h2d(world.cursor.ptr, np.array([SENTINEL], dtype=np.uint64))
    world.eng.sync()
    assert world.call(enc, rows=0) == OK, gpu.lib().gcn10_gpu_last_error().decode()
    world.eng.sync()
    assert int(world.eng.download(world.cursor.ptr, (1,), dtype=np.uint64)[0]) == SENTINEL
    world.good_call(enc)


def test_arena_bounds():
    L = gpu.lib()
    assert L.gcn10_gpu_deflate_arena_bound(256, 256, 1) == 65552 + 4096
    assert L.gcn10_gpu_deflate_arena_bound(257, 256, 2) == 4 * 65552 + 2 * 4096
    assert L.gcn10_gpu_deflate_arena_bound(0, 256, 1) == 0
    assert L.gcn10_gpu_lzw_arena_bound(256, 256, 1) == 82032 + 4096
    assert L.gcn10_gpu_lzw_arena_bound(257, 256, 2) == 4 * 82032 + 2 * 4096
    assert L.gcn10_gpu_lzw_arena_bound(0, 256, 1) == 0
