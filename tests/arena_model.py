"""The layout contract of the tile encoders' arena (include/gcn10_gpu.h, gcn10_gpu_deflate_strip), stated once
more in plain Python: where every stream lies, what the table and the cursor say, which bytes the encoder has to
write as zeros and which it must leave alone.  No GPU, no code shared with the kernels.

The rule:
  * streams lie in index order (raster-major, tiles of a raster row-major), each in a slot of ceil16(size) bytes;
  * an alias (this raster's tile is an earlier raster's stream) takes no room, its table entry is its original's;
  * raster 0's extent starts at 0, every later raster's at the next multiple of seg_align behind the previous
    raster's last slot; the cursor is the end of the last raster's last slot, not aligned;
  * a stream fits if and only if offset + ceil16(size) <= arena_cap, otherwise its entry is (0xffffffff, 0);
  * zeros: every fitting stream's slot tail, the pad behind every raster up to the next raster's extent, and behind
    the last raster up to the next multiple of seg_align -- each written in whole 16-byte units that end at or
    before arena_cap;
  * every other byte of the arena, and every byte behind arena_cap, keeps what it held.
Where a stream that does not fit would have lain is left unspecified.
"""
import numpy as np

NO_ROOM = (0xFFFFFFFF, 0)


def ceil_to(x, a):
    return -(-x // a) * a


class Layout:
    """table: uint32[n_rasters, tiles, 2]; cursor; starts / ends: every raster's extent; streams, zeros,
    unspecified: lists of byte ranges (a, b), a < b."""

    def __init__(self):
        self.table = None
        self.cursor = 0
        self.starts, self.ends = [], []
        self.streams, self.zeros, self.unspecified = [], [], []


def _whole_units(a, b, cap):
    """[a, b) cut to the whole 16-byte units from a on that end at or before cap (None if there is none)."""
    b = min(b, cap)
    if b <= a:
        return None
    b = a + (b - a) // 16 * 16
    return (a, b) if b > a else None


def layout(sizes, alias_of, seg_align, arena_cap):
    """sizes[r][t]: stream bytes of tile t of raster r; alias_of[r][t]: None, or the earlier raster whose stream of
    tile t this one shares (alias_of=None: no aliases).  Returns the Layout the encoder must produce."""
    n, tiles = len(sizes), len(sizes[0])
    assert seg_align >= 16 and seg_align & (seg_align - 1) == 0
    lay = Layout()
    table = np.zeros((n, tiles, 2), np.uint32)
    at = 0
    for r in range(n):
        assert len(sizes[r]) == tiles
        if r:
            at = ceil_to(at, seg_align)
        lay.starts.append(at)
        for t in range(tiles):
            src = None if alias_of is None else alias_of[r][t]
            if src is not None:
                assert 0 <= src < r, "an alias names an earlier raster"
                table[r, t] = table[src, t]
                continue
            size = int(sizes[r][t])
            assert size > 0
            slot = ceil_to(size, 16)
            if at + slot <= arena_cap:
                table[r, t] = (at, size)
                lay.streams.append((at, at + size))
                if slot > size:
                    lay.zeros.append((at + size, at + slot))
            else:
                table[r, t] = NO_ROOM
                lay.unspecified.append((at, at + slot))
            at += slot
        lay.ends.append(at)
    lay.cursor = at
    for r in range(n):
        pad = _whole_units(lay.ends[r], lay.starts[r + 1] if r + 1 < n else ceil_to(lay.ends[r], seg_align), arena_cap)
        if pad:
            lay.zeros.append(pad)
    lay.table = table
    return lay


def check_table(lay, table, cursor):
    """The encoder's table and cursor are the model's."""
    got = np.asarray(table).reshape(lay.table.shape)
    if not np.array_equal(got, lay.table):
        r, t = [int(v[0]) for v in np.nonzero((got != lay.table).any(axis=2))]
        raise AssertionError("table entry (raster %d, tile %d) is %s, the layout rule says %s"
                             % (r, t, tuple(got[r, t].tolist()), tuple(lay.table[r, t].tolist())))
    assert int(cursor) == lay.cursor, "cursor %d, the layout rule says %d" % (int(cursor), lay.cursor)


def _first(mask, a):
    return a + int(np.flatnonzero(mask)[0])


def check_image(lay, image, arena_cap, poison=0xA5):
    """image: the arena and the guard behind it (arena_cap + guard bytes), downloaded after an encoder ran on it
    poisoned.  Every zero range is zero; every byte at or beyond arena_cap, and every byte inside it that belongs to
    no stream, no zero range and no slot of a stream that did not fit, is still poison."""
    image = np.asarray(image, np.uint8)
    assert len(image) >= arena_cap
    for a, b in lay.zeros:
        assert b <= arena_cap, "the model itself: a zero range ends behind the arena"
        part = image[a:b]
        if part.any():
            raise AssertionError("byte %d is 0x%02x: [%d, %d) must be zeros" % (_first(part != 0, a), part[part != 0][0], a, b))
    claimed = sorted(lay.streams + lay.zeros + lay.unspecified)
    at = 0
    for a, b in claimed + [(arena_cap, arena_cap)]:
        a, b = min(a, arena_cap), min(b, arena_cap)
        assert a >= at, "the model itself: ranges [.., %d) and [%d, ..) overlap" % (at, a)
        part = image[at:a]
        if (part != poison).any():
            raise AssertionError("byte %d is 0x%02x: [%d, %d) belongs to no stream and no pad and must be untouched"
                                 % (_first(part != poison, at), part[part != poison][0], at, a))
        at = b
    part = image[arena_cap:]
    if (part != poison).any():
        raise AssertionError("byte %d behind arena_cap = %d is 0x%02x: written out of bounds"
                             % (_first(part != poison, arena_cap), arena_cap, part[part != poison][0]))


def check(lay, table, cursor, image, arena_cap, poison=0xA5):
    check_table(lay, table, cursor)
    check_image(lay, image, arena_cap, poison)
