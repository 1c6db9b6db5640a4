#!/usr/bin/env python3
"""Kernel-level timing of the area means on a coarser grid (gcn10_gpu_aggregate) against its yardstick, in one process,
on the 36000 x 36000 blocks of bench.synth_block (patterns patches and natural):

  (a) gcn10_gpu_aggregate, all 18 rasters, f = 25 and f = 100, the block in one call (what the host program
      launches) or in bands of --band-rows rows;
  (b) gcn10_gpu_cn_strip, all 18 rasters, on the same landcover in strips of --rows rows into 18 full-size rasters:
      the same two 16-byte table gathers per pixel, plus 23 GB of stores that (a) does not make;
  (c) gcn10_gpu_stream_copy of the block's 1.296 GB of landcover: what the device sustains for 1 byte read : 1 byte
      written in this very run.  read_bound_ms is the time the landcover alone takes at that rate (bytes read + bytes
      written per second), the floor of (a).

Every figure is the time between two events around the launches of one block, after one warm-up block; min and median
of --reps.  One JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from gcn10_amd import gpu, host  # noqa: E402


def timed(e, fn, reps):
    e0, e1 = e.event_create(), e.event_create()
    ms = []
    for _rep in range(reps + 1):            # the first one warms up
        e.event_record(e0)
        fn()
        e.event_record(e1)
        e.event_sync(e1)
        ms.append(e.elapsed_ms(e0, e1))
    e.event_destroy(e0)
    e.event_destroy(e1)
    return {"min_ms": round(min(ms[1:]), 3), "median_ms": round(float(np.median(ms[1:])), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", default="patches,natural")
    ap.add_argument("--size", type=int, default=36000)
    ap.add_argument("--rows", type=int, default=2304, help="rows per strip of leg (b)")
    ap.add_argument("--band-rows", type=int, default=0,
                    help="rows per call of leg (a), rounded down to whole cell rows (0 = the block in one call, as the "
                         "host program launches it)")
    ap.add_argument("--factors", default="25,100")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    S = a.size
    factors = [int(f) for f in a.factors.split(",")]
    tables = host.load_all_lookup_tables(os.path.join(ROOT, "tests", "golden", "lookups"))
    res = {"size": S, "rows": a.rows, "band_rows": a.band_rows, "reps": a.reps, "rasters": 18, "patterns": {}}
    with gpu.Engine(0) as e:
        e.set_tables(tables)
        res["device"] = e.device_info()["name"]
        outs = e.alloc(18 * S * S)
        small = e.alloc(18 * (-(-S // min(factors))) ** 2)
        copy_dst = e.alloc(S * S)
        for pattern in a.patterns.split(","):
            esa, gt, coarse, sgt = bench.synth_block(1, S, pattern)
            hsy, hsx = coarse.shape
            ci, cj = host.build_index_maps(gt, sgt, S, S, hsx, hsy)
            bufs = [e.upload(x) for x in (esa, coarse, ci, cj)]
            del esa
            e.prepare_tile(bufs[1].ptr, hsx, hsy, bufs[2].ptr, S)
            one = {}

            def strips():
                for y0 in range(0, S, a.rows):
                    rows = min(a.rows, S - y0)
                    e.cn_strip(bufs[0].at(y0 * S), S, rows, bufs[3].at(4 * y0), 3, 0x1FF,
                               [outs.at(r * S * S + y0 * S) for r in range(18)])

            def aggregate(f):
                Wa, Ha = -(-S // f), -(-S // f)
                band = max((a.band_rows or S + f) // f, 1) * f
                for y0 in range(0, S, band):
                    rows = min(band, S - y0)
                    e.aggregate(bufs[0].at(y0 * S), S, rows, bufs[3].at(4 * y0), 0, S, f, 3, 0x1FF,
                                [small.at(q * Wa * Ha + (y0 // f) * Wa) for q in range(18)], Wa)

            one["copy"] = timed(e, lambda: e.stream_copy(bufs[0].ptr, copy_dst.ptr, S * S), a.reps)
            rate = 2.0 * S * S / (one["copy"]["min_ms"] * 1e-3)            # bytes read + written per second
            one["copy"]["gb_per_s"] = round(rate / 1e9, 1)
            one["read_bound_ms"] = round(S * S / rate * 1e3, 3)
            one["cn_strip"] = timed(e, strips, a.reps)
            for f in factors:
                t = timed(e, lambda f=f: aggregate(f), a.reps)
                t["ratio_to_cn_strip"] = round(t["min_ms"] / one["cn_strip"]["min_ms"], 3)
                t["landcover_gb_per_s"] = round(S * S / (t["min_ms"] * 1e-3) / 1e9, 1)
                one["aggregate_x%d" % f] = t
            res["patterns"][pattern] = one
            e.sync()
            for b in bufs:
                b.close()
        for b in (outs, small, copy_dst):
            b.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
