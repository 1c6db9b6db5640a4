#!/usr/bin/env python3
"""Kernel-level timing of the sums on a model grid (gcn10_gpu_grid_sums) against its yardstick, in one process, on the
36000 x 36000 blocks of bench.synth_block (patterns patches and natural), all 18 rasters:

  (a) gcn10_gpu_grid_sums with cells of exactly 25 px aligned to the block's origin: the cells of --aggregate 25;
  (b) gcn10_gpu_aggregate, f = 25, on the same buffers: the yardstick;
  (c) gcn10_gpu_grid_sums with cells of 25.6 px (25 and 26 px in turn), of 120 px and of 1200 px;
  (d) gcn10_gpu_stream_copy of the block's 1.296 GB of landcover: what the device sustains in this very run.

Every figure is the time between two events around the launches of one block (for (a) and (c): the memset of the
pairs, the kernel, and gcn10_gpu_grid_finish; the kernel alone is reported too), after one warm-up block; min and
median of --reps.  The means of (a) are compared with the bytes of (b).  One JSON line; --out also writes it to a
file."""
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


def cell_map(n, width):
    """cell of every pixel for cells of `width` pixels from pixel 0 on: centre i + 0.5 in [k width, (k + 1) width)"""
    return np.floor((np.arange(n) + 0.5) / width).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", default="patches,natural")
    ap.add_argument("--size", type=int, default=36000)
    ap.add_argument("--cells", default="25,25.6,120,1200", help="cell sizes in pixels; the first is leg (a)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    S = a.size
    widths = [float(c) for c in a.cells.split(",")]
    f = int(widths[0])
    assert f == widths[0] and 2 <= f <= 256, "leg (a) is compared with gcn10_gpu_aggregate: a whole factor"
    tables = host.load_all_lookup_tables(os.path.join(ROOT, "tests", "golden", "lookups"))
    res = {"size": S, "reps": a.reps, "rasters": 18, "patterns": {}}
    n_max = max(int(cell_map(S, w).max()) + 1 for w in widths)
    with gpu.Engine(0) as e:
        e.set_tables(tables)
        res["device"] = e.device_info()["name"]
        acc = e.alloc(18 * n_max * n_max * 16)
        means = e.alloc(18 * n_max * n_max)
        agg = e.alloc(18 * n_max * n_max)
        copy_dst = e.alloc(S * S)
        for pattern in a.patterns.split(","):
            esa, gt, coarse, sgt = bench.synth_block(1, S, pattern)
            hsy, hsx = coarse.shape
            ci, cj = host.build_index_maps(gt, sgt, S, S, hsx, hsy)
            bufs = [e.upload(x) for x in (esa, coarse, ci, cj)]
            del esa
            e.prepare_tile(bufs[1].ptr, hsx, hsy, bufs[2].ptr, S)
            one = {}

            def sums(m, n):
                e.grid_sums(bufs[0].ptr, S, S, bufs[3].ptr, m.ptr, m.ptr, n, n, 3, 0x1FF, acc.ptr)

            def whole(m, n):
                e.memset(acc.ptr, 0, 18 * n * n * 16)
                sums(m, n)
                e.grid_finish(acc.ptr, 18, n * n, means.ptr, None, 0, None)

            def aggregate():
                Wa = -(-S // f)
                e.aggregate(bufs[0].ptr, S, S, bufs[3].ptr, 0, S, f, 3, 0x1FF,
                            [agg.at(q * Wa * Wa) for q in range(18)], Wa)

            one["copy"] = timed(e, lambda: e.stream_copy(bufs[0].ptr, copy_dst.ptr, S * S), a.reps)
            rate = 2.0 * S * S / (one["copy"]["min_ms"] * 1e-3)            # bytes read + written per second
            one["copy"]["gb_per_s"] = round(rate / 1e9, 1)
            one["read_bound_ms"] = round(S * S / rate * 1e3, 3)
            one["aggregate_x%d" % f] = timed(e, aggregate, a.reps)
            base = None
            for w in widths:
                m_host = cell_map(S, w)
                n = int(m_host.max()) + 1
                m = e.upload(m_host)
                t = timed(e, lambda m=m, n=n: whole(m, n), a.reps)
                t["kernel"] = timed(e, lambda m=m, n=n: sums(m, n), a.reps)
                t["cells"] = n * n
                if base is None:
                    base = t
                    t["ratio_to_aggregate"] = round(t["min_ms"] / one["aggregate_x%d" % f]["min_ms"], 3)
                    t["kernel"]["ratio_to_aggregate"] = round(t["kernel"]["min_ms"] / one["aggregate_x%d" % f]["min_ms"], 3)
                    whole(m, n)
                    e.sync()
                    t["means_equal_aggregate"] = bool(np.array_equal(e.download(means.ptr, (18 * n * n,)),
                                                                     e.download(agg.ptr, (18 * n * n,))))
                else:
                    t["ratio_to_first"] = round(t["min_ms"] / base["min_ms"], 3)
                    t["kernel"]["ratio_to_first"] = round(t["kernel"]["min_ms"] / base["kernel"]["min_ms"], 3)
                t["landcover_gb_per_s"] = round(S * S / (t["kernel"]["min_ms"] * 1e-3) / 1e9, 1)
                one["grid_%gpx" % w] = t
                e.sync()
                m.close()
            res["patterns"][pattern] = one
            e.sync()
            for b in bufs:
                b.close()
        for b in (acc, means, agg, copy_dst):
            b.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
