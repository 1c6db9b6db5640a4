"""Writes tests/golden/deflate/: zlib streams made by libdeflate (the encoder GDAL uses for DEFLATE tiles when it
has it), which writes forms zlib's encoder never does (length-3 matches far back, precode runs across HLIT, ...).

    python tests/golden/make_deflate_corpus.py

Tiles of 256 x 256 and 1024 x 1024 bytes, CN-like textures, levels 1 / 6 / 9 / 12.  manifest.json lists every
stream with the size and SHA-256 of what it decodes to; the tests read only these files (libdeflate need not be
installed where they run)."""
import ctypes
import ctypes.util
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "deflate")
LEVELS = (1, 6, 9, 12)
CLASSES = np.array([10, 20, 30, 40, 50, 60, 70, 80, 90, 95, 100], np.uint8)
CN_VALUES = np.array([0, 15, 30, 35, 41, 48, 51, 55, 59, 62, 68, 72, 77, 83, 98, 255], np.uint8)
# (rows, columns) per texture; "words" (repeats of 3-pixel words from a pool of 1200) is the texture for which the
# near-optimal parser writes length-3 matches more than 4096 back
SHAPES = {"patchy": [(256, 256), (1024, 1024)], "natural": [(256, 256), (1024, 1024)], "iid": [(256, 256)],
          "constant": [(256, 256), (1024, 1024)], "words": [(64, 256)]}


def load_libdeflate():
    """libdeflate through ctypes, or None where it is not installed."""
    for name in ("libdeflate.so.0", ctypes.util.find_library("deflate")):
        if not name:
            continue
        try:
            lib = ctypes.CDLL(name)
        except OSError:
            continue
        lib.libdeflate_alloc_compressor.restype = ctypes.c_void_p
        lib.libdeflate_alloc_compressor.argtypes = [ctypes.c_int]
        lib.libdeflate_zlib_compress.restype = ctypes.c_size_t
        lib.libdeflate_zlib_compress.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                                 ctypes.c_size_t]
        lib.libdeflate_free_compressor.argtypes = [ctypes.c_void_p]
        lib.libdeflate_alloc_decompressor.restype = ctypes.c_void_p
        lib.libdeflate_zlib_decompress.restype = ctypes.c_int
        lib.libdeflate_zlib_decompress.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                                   ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
        lib.libdeflate_free_decompressor.argtypes = [ctypes.c_void_p]
        return lib
    return None


def compress(lib, raw, level):
    c = lib.libdeflate_alloc_compressor(level)
    assert c
    cap = len(raw) + len(raw) // 8 + 1024
    out = ctypes.create_string_buffer(cap)
    n = lib.libdeflate_zlib_compress(c, raw, len(raw), out, cap)
    lib.libdeflate_free_compressor(c)
    assert n > 0
    return out.raw[:n]


def decompress_exact(lib, stream, size):
    """libdeflate's zlib decoder into a buffer of exactly `size` bytes, as libtiff decodes a tile; None when it
    refuses the stream or it does not fill the buffer."""
    d = lib.libdeflate_alloc_decompressor()
    out = ctypes.create_string_buffer(max(size, 1))
    got = ctypes.c_size_t(0)
    rc = lib.libdeflate_zlib_decompress(d, bytes(stream), len(stream), out, size, ctypes.byref(got))
    lib.libdeflate_free_decompressor(d)
    return out.raw[:size] if rc == 0 and got.value == size else None


def texture(kind, h, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "constant":
        return np.full((n, n), 80, np.uint8)
    if kind == "iid":                   # i.i.d. over the CN values: ~4 bits per pixel
        return rng.choice(CN_VALUES, size=(n, n))
    if kind == "words":
        words = rng.integers(0, 256, (1200, 3), dtype=np.uint8)
        return words[rng.integers(0, 1200, h * n // 3 + 1)].reshape(-1)[:h * n].reshape(h, n)
    if kind == "patchy":                # 32-px patches of landcover classes
        small = rng.integers(0, len(CLASSES), size=(n // 32, n // 32))
        return CLASSES[np.kron(small, np.ones((32, 32), np.int64))]
    if kind == "natural":               # classes of a field with detail at several scales: ragged patch edges
        f = np.zeros((n, n))
        for s, wgt in ((128, 1.0), (32, 0.5), (8, 0.25)):
            small = rng.standard_normal((n // s + 1, n // s + 1))
            f += wgt * np.kron(small, np.ones((s, s)))[:n, :n]
        q = np.clip(((f + 2.0) * 2.5).astype(np.int64), 0, len(CLASSES) - 1)
        return CLASSES[q]
    raise ValueError(kind)


def main():
    lib = load_libdeflate()
    if lib is None:
        sys.exit("libdeflate is not installed")
    os.makedirs(OUT, exist_ok=True)
    manifest = []
    for kind, shapes in SHAPES.items():
        for h, n in shapes:
            raw = np.ascontiguousarray(texture(kind, h, n, seed=n + len(kind))).tobytes()
            for level in LEVELS:
                name = "%s_%dx%d_L%d.zz" % (kind, h, n, level)
                st = compress(lib, raw, level)
                with open(os.path.join(OUT, name), "wb") as f:
                    f.write(st)
                manifest.append({"file": name, "texture": kind, "rows": h, "width": n, "level": level, "size": len(raw),
                                 "sha256": hashlib.sha256(raw).hexdigest()})
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")
    total = sum(os.path.getsize(os.path.join(OUT, m["file"])) for m in manifest)
    print("%d streams, %d bytes" % (len(manifest), total))


if __name__ == "__main__":
    main()
