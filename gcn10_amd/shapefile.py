"""A small polygon-shapefile writer (.shp / .shx / .dbf) for zone files: the tests of the zonal run mode and
tools/bench_zonal.py make their zones with it.  The reader is gcn10_zones_open (host.Zones)."""
import struct


def write_zone_shapefile(base, zones, shape_type=5, id_field="ID", raw_records=None):
    """zones: list of (id, rings) -> base.shp / .shx / .dbf; rings = list of [(x, y), ...] (closed here when open), or
    None for a null shape.  shape_type 5 (Polygon) or 15 (PolygonZ, with zero Z and M).  raw_records: {index: bytes}
    replaces a record's content (to write other shape types)."""
    recs = []
    for i, (_id, rings) in enumerate(zones):
        if raw_records and i in raw_records:
            recs.append(raw_records[i])
            continue
        if rings is None:
            recs.append(struct.pack("<i", 0))
            continue
        rings = [list(r) + ([r[0]] if tuple(r[0]) != tuple(r[-1]) else []) for r in rings]
        pts = [p for r in rings for p in r]
        xs, ys = [p[0] for p in pts], [p[1] for p in pts]
        c = struct.pack("<i4d2i", shape_type, min(xs), min(ys), max(xs), max(ys), len(rings), len(pts))
        at = 0
        for r in rings:
            c += struct.pack("<i", at)
            at += len(r)
        c += b"".join(struct.pack("<2d", float(x), float(y)) for x, y in pts)
        if shape_type == 15:
            c += struct.pack("<2d", 0, 0) + struct.pack("<%dd" % len(pts), *([0.0] * len(pts)))
            c += struct.pack("<2d", 0, 0) + struct.pack("<%dd" % len(pts), *([0.0] * len(pts)))
        recs.append(c)
    total = 100 + sum(8 + len(c) for c in recs)

    def header(length_bytes):
        return (struct.pack(">i5ii", 9994, 0, 0, 0, 0, 0, length_bytes // 2) +
                struct.pack("<ii4d4d", 1000, shape_type, -180.0, -90.0, 180.0, 90.0, 0, 0, 0, 0))

    with open(base + ".shp", "wb") as f, open(base + ".shx", "wb") as fx:
        f.write(header(total))
        fx.write(header(100 + 8 * len(recs)))
        pos = 100
        for i, c in enumerate(recs):
            f.write(struct.pack(">ii", i + 1, len(c) // 2) + c)
            fx.write(struct.pack(">ii", pos // 2, len(c) // 2))
            pos += 8 + len(c)
    fields = [(b"fid", b"N", 10), (id_field.encode(), b"N", 12), (b"NAME", b"C", 8)]
    hdr_len = 32 + 32 * len(fields) + 1
    rec_len = 1 + sum(f[2] for f in fields)
    with open(base + ".dbf", "wb") as f:
        f.write(struct.pack("<BBBBIHH20x", 3, 124, 1, 1, len(zones), hdr_len, rec_len))
        for name, typ, ln in fields:
            f.write(name.ljust(11, b"\0") + typ + b"\0" * 4 + bytes([ln, 0]) + b"\0" * 14)
        f.write(b"\x0d")
        for i, z in enumerate(zones):
            f.write(b" " + str(i + 1).rjust(10).encode() + str(z[0]).rjust(12).encode() + b"zone".ljust(8))
        f.write(b"\x1a")
