"""An independent checker of the Cloud Optimized GeoTIFF layout the writer promises (gcn10_tiff_create_cog):
GDAL's ghost area, IFDs before the data, level sizes, NewSubfileType, level-before-level data order and
row-major increasing tile offsets.  ``check_cog(path)`` raises AssertionError naming the broken rule and returns
the parsed IFDs."""
import math
import struct

GHOST_BODY = b"LAYOUT=IFDS_BEFORE_DATA\nBLOCK_ORDER=ROW_MAJOR\nKNOWN_INCOMPATIBLE_EDITION=NO\n"
TYPE_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 1, 8: 2, 9: 4, 10: 8, 11: 4, 12: 8, 16: 8}
TYPE_FMT = {1: "B", 2: "B", 3: "H", 4: "I", 12: "d", 16: "Q"}
GEO_TAGS = {33550, 33922, 34264, 34735, 34736, 34737}


def expected_levels(W, H, block=256):
    """GDAL's COG rule: the smallest k >= 0 with ceil(W/2^k) <= block and ceil(H/2^k) <= block."""
    k = 0
    while math.ceil(W / 2 ** k) > block or math.ceil(H / 2 ** k) > block:
        k += 1
    return k


def read_ifds(data: bytes):
    """[(ifd_offset, {tag: (type, count, values or value_offset, value_byte_ranges)})] in chain order."""
    assert data[:4] == b"II*\x00", "not a little-endian classic TIFF"
    pos = struct.unpack_from("<I", data, 4)[0]
    out, seen = [], set()
    while pos:
        assert pos not in seen and pos % 2 == 0 and pos + 2 <= len(data), "bad IFD offset %d" % pos
        seen.add(pos)
        n = struct.unpack_from("<H", data, pos)[0]
        tags, ranges = {}, []
        last = -1
        for i in range(n):
            tag, typ, cnt, val = struct.unpack_from("<HHII", data, pos + 2 + 12 * i)
            assert tag > last, "IFD tags not ascending"
            last = tag
            size = TYPE_SIZE[typ] * cnt
            at = pos + 2 + 12 * i + 8 if size <= 4 else val
            if size > 4:
                assert at + size <= len(data), "tag %d value beyond the file" % tag
                ranges.append((at, at + size))
            raw = data[at:at + size]
            vals = list(struct.unpack("<%d%s" % (cnt, TYPE_FMT[typ]), raw)) if typ in TYPE_FMT else raw
            tags[tag] = vals
        end = pos + 2 + 12 * n + 4
        out.append((pos, end, tags, ranges))
        pos = struct.unpack_from("<I", data, pos + 2 + 12 * n)[0]
    return out


def check_cog(path, n_levels=None, compression=None):
    with open(path, "rb") as f:
        data = f.read()
    # ghost area
    first = b"GDAL_STRUCTURAL_METADATA_SIZE="
    assert data[8:8 + len(first)] == first, "no ghost area at offset 8"
    nl = data.index(b"\n", 8)
    line = data[8:nl + 1]
    assert line.endswith(b" bytes\n") and len(line) == len(first) + 6 + 7, "bad first ghost line %r" % line
    size = int(line[len(first):len(first) + 6])
    body = data[nl + 1:nl + 1 + size]
    assert body == GHOST_BODY, "ghost body %r" % body
    ghost_end = nl + 1 + size

    ifds = read_ifds(data)
    main = ifds[0][2]
    W, H = main[256][0], main[257][0]
    L = expected_levels(W, H)
    assert len(ifds) == L + 1, "%d IFDs for %dx%d, want %d" % (len(ifds), W, H, L + 1)
    if n_levels is not None:
        assert L == n_levels
    assert 254 not in main or main[254][0] == 0, "main IFD is not full resolution"
    comp = main[259][0]
    if compression is not None:
        assert comp == compression, "Compression %d" % comp
    # IFDs with their values before all tile data
    meta_end = max(max([e for _p, e, _t, _r in ifds]), max([b for _p, _e, _t, rr in ifds for _a, b in rr] or [0]))
    meta_start = min(p for p, _e, _t, _r in ifds)
    assert meta_start >= ghost_end, "an IFD overlaps the ghost area"
    for k, (_pos, _end, tags, _r) in enumerate(ifds):
        if k > 0:
            assert tags.get(254, [0])[0] == 1, "level %d: NewSubfileType != 1" % k
            assert not GEO_TAGS & set(tags), "level %d has geo tags" % k
        w, h = tags[256][0], tags[257][0]
        assert (w, h) == (math.ceil(W / 2 ** k), math.ceil(H / 2 ** k)), "level %d is %dx%d" % (k, w, h)
        assert tags[322][0] == 256 and tags[323][0] == 256, "level %d tiles are not 256x256" % k
        assert tags[259][0] == comp, "level %d Compression differs" % k
        assert tags[258][0] == 8 and tags[277][0] == 1
        n = math.ceil(w / 256) * math.ceil(h / 256)
        offs, cnts = tags[324], tags[325]
        assert len(offs) == n and len(cnts) == n, "level %d: %d tiles, want %d" % (k, len(offs), n)
        for i in range(n):
            assert cnts[i] > 0 and offs[i] >= meta_end, "level %d tile %d lies before the data" % (k, i)
            assert offs[i] + cnts[i] <= len(data), "level %d tile %d beyond the file" % (k, i)
            if i:
                assert offs[i] > offs[i - 1], "level %d: tile offsets not increasing at %d" % (k, i)
    # level L's data first, full resolution last
    for k in range(L, 0, -1):
        coarse, fine = ifds[k][2], ifds[k - 1][2]
        last = max(o + c for o, c in zip(coarse[324], coarse[325]))
        assert last <= min(fine[324]), "level %d data is not wholly before level %d's" % (k, k - 1)
    return ifds


def tile_bytes(path, ifds, level, i):
    tags = ifds[level][2]
    with open(path, "rb") as f:
        f.seek(tags[324][i])
        return f.read(tags[325][i])
