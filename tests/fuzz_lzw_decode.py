#!/usr/bin/env python3
"""Randomised check of the GPU LZW decoder (not collected by pytest; run it on a GPU box:
`python tests/fuzz_lzw_decode.py --streams 20000`).  Every stream is written code by code (tests/lzw_model.py):
at each step a literal, a random live entry, one of the newest three entries, KwKwK or a Clear; now and then an
invalid code or a truncated stream; out_len below, at or above the decoded size.  Every stream must come out of
gcn10_gpu_inflate_tiles as the reference decoder gives it, bytes and status.  Exit code 1 on any difference.
`--model-only` draws the streams and reports what they reach without a GPU."""
import argparse
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.lzw_model import FIRST, LzwError, LzwWriter, lzw_decode_ref, width_of  # noqa: E402

GUARD = 8               # zero columns / rows around every tile's window in the destination
TILE_LZW = 4


def chunk_width(out_len, limit=2048):
    """The largest width up to `limit` that divides out_len (1 is fine)."""
    for w in range(min(out_len, limit), 0, -1):
        if out_len % w == 0:
            return w
    return 1


def decode_tiles(engine, streams, out_lens, flags=None):
    """One launch: stream i is a chunk of out_lens[i] bytes in rows of a width that divides it, placed whole in
    its own band of the destination with GUARD zero pixels around it.  Returns (chunks, status); asserts that
    nothing was written outside the windows."""
    n = len(streams)
    flags = flags if flags is not None else [TILE_LZW] * n
    cws = [chunk_width(max(L, 1)) for L in out_lens]
    rows = [L // cw for L, cw in zip(out_lens, cws)]
    W = max(cws) + 2 * GUARD
    ys, y = [], GUARD
    for r in rows:
        ys.append(y)
        y += r + GUARD
    wins = [(0, 0, cws[i] if rows[i] else 0, rows[i], GUARD, ys[i]) for i in range(n)]
    out, status = engine.inflate_tiles(streams, cws, [max(r, 1) for r in rows], wins, (y, W), flags=flags,
                                       out_lens=list(out_lens))
    chunks = []
    for i in range(n):
        chunks.append(out[ys[i]:ys[i] + rows[i], GUARD:GUARD + cws[i]].reshape(-1).copy())
        out[ys[i]:ys[i] + rows[i], GUARD:GUARD + cws[i]] = 0
    assert not out.any(), "bytes written outside the tiles' windows"
    return chunks, status


def draw(rng):
    """One stream and its out_len."""
    w = LzwWriter(clear=rng.random() < 0.9)
    n_codes = int(2 ** rng.uniform(0, 12.3))                # 1 .. 5000, half of them below 71
    p_lit = rng.uniform(0.15, 0.95)
    p_clear = rng.choice((0.0, 0.0, 0.001, 0.004, 0.03))
    bad_at = rng.randrange(n_codes) if rng.random() < 0.07 else -1
    for i in range(n_codes):
        if i == bad_at:
            top = (1 << width_of(w.n)) - 1
            if w.prev is None:
                w.raw(FIRST + rng.randrange(200))           # a first code that is not a literal
            elif w.next + 1 <= top:
                w.raw(rng.randrange(w.next + 1, top + 1))   # beyond the dictionary
            else:
                w.clear()
                w.raw(FIRST)
            break
        r = rng.random()
        if r < p_clear:
            w.clear()
        elif w.prev is None or w.next == FIRST or r < p_clear + p_lit:
            w.lit(rng.randrange(256) if rng.random() < 0.7 else rng.randrange(4))
        else:
            r = rng.random()
            if r < 0.15 and not w.full:
                w.kwkwk()
            elif r < 0.45:
                w.code(max(FIRST, w.next - 1 - rng.randrange(3)))
            else:
                w.code(rng.randrange(FIRST, w.next))
    if rng.random() < 0.85:
        w.eoi()
    stream = w.stream()
    if rng.random() < 0.06 and len(stream) > 1:
        stream = stream[:rng.randrange(len(stream))]
    size = max(len(w.out), 1)
    r = rng.random()
    if r < 0.35:
        # inside one of the last codes (since the last Clear) that is longer than a byte, where there is one
        ends = w.starts[1:] + [len(w.out)]
        inside = [(a, b) for a, b in list(zip(w.starts, ends))[-12:] if b - a > 1]
        a, b = rng.choice(inside) if inside else (size - 1, size)
        out_len = max(1, rng.randrange(a + 1, b) if b - a > 1 else a)
    elif r < 0.7:
        out_len = size
    else:
        out_len = size + rng.randrange(1, 300)
    return stream, out_len


def run(seed=1, streams=512, engine=None, batch=512, verbose=True):
    """Draws `streams` streams; with an engine, decodes them on the GPU (batch per launch) and compares.
    Returns a dict: n, refused, cut (streams whose last code out_len cuts), wide (streams that reach 11-bit
    codes), early_eoi, bad (differences: (index, what))."""
    rng = random.Random(seed)
    res = dict(n=0, refused=0, cut=0, wide=0, early_eoi=0, bad=[])
    todo = []
    for k in range(streams):
        stream, out_len = draw(rng)
        try:
            want, tr = lzw_decode_ref(stream, out_len, trace=True)
            res["cut"] += bool(tr.codes) and tr.codes[-1].cut
            res["wide"] += any(c.width >= 11 for c in tr.codes)
            res["early_eoi"] += bool(tr.eois) and tr.eois[0].pos < out_len
        except LzwError as e:
            want = e.status
            res["refused"] += 1
        res["n"] += 1
        todo.append((k, stream, out_len, want))
        if engine is not None and (len(todo) == batch or k == streams - 1):
            chunks, status = decode_tiles(engine, [t[1] for t in todo], [t[2] for t in todo])
            for (i, stream, out_len, want), got, st in zip(todo, chunks, status):
                if isinstance(want, int):
                    if int(st) != want:
                        res["bad"].append((i, "status %d, the model refuses it with %d" % (int(st), want)))
                elif int(st) != 0:
                    res["bad"].append((i, "status %d, the model decodes it" % int(st)))
                elif got.tobytes() != want:
                    first = int(np.flatnonzero(got != np.frombuffer(want, np.uint8))[0])
                    res["bad"].append((i, "byte %d of %d differs" % (first, out_len)))
            todo = []
            if verbose:
                print("... %d streams, %d differences" % (res["n"], len(res["bad"])), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--model-only", action="store_true", help="draw and count, no GPU")
    a = ap.parse_args()
    if a.model_only:
        res = run(a.seed, a.streams, None)
    else:
        from gcn10_amd import gpu
        with gpu.Engine(0) as e:
            res = run(a.seed, a.streams, e)
    for i, what in res["bad"][:20]:
        print("DIFFERENCE: seed %d stream %d: %s" % (a.seed, i, what))
    print("seed %d: streams %d, refused by the model %d, cut codes %d, reach 11-bit codes %d, early EOI %d, "
          "differences %d" % (a.seed, res["n"], res["refused"], res["cut"], res["wide"], res["early_eoi"],
                              len(res["bad"])))
    sys.exit(1 if res["bad"] else 0)


if __name__ == "__main__":
    main()
