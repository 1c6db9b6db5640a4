#!/usr/bin/env python3
"""Kernel-level timing of the weighted sums on a model grid (gcn10_gpu_grid_sums_weighted) against the mean-only path,
in one process, on the 36000 x 36000 blocks of bench.synth_block (patterns patches and natural), all 18 rasters, cells
of 25 px and of 1200 px:

  (a) the yardstick: memset of the pairs, gcn10_gpu_grid_sums, gcn10_gpu_grid_finish;
  (b) the weighted trio on the same cells: memset of the triples, gcn10_gpu_grid_sums_weighted,
      gcn10_gpu_grid_finish_weighted, with the runoff table of --storm;
  (c) gcn10_gpu_stream_copy of the block's 1.296 GB of landcover: what the device sustains in this very run.

Every figure is the time between two events around the launches of one block, after one warm-up block; min and median
of --reps; the two sums kernels alone are reported too.  The weighted pass does three gathers where the yardstick does
one and reads the same bytes: three launches of the yardstick's kernel are the trivial bound.  The triples' first two
words and the means are compared with the yardstick's.  One JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from gcn10_amd import gpu, host  # noqa: E402
from tools.bench_grid import cell_map, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", default="patches,natural")
    ap.add_argument("--size", type=int, default=36000)
    ap.add_argument("--cells", default="25,1200", help="cell sizes in pixels")
    ap.add_argument("--storm", default="50,0.2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    S = a.size
    widths = [float(c) for c in a.cells.split(",")]
    P, lam = host.parse_storm(a.storm)
    q = host.runoff_table(P, lam)
    tables = host.load_all_lookup_tables(os.path.join(ROOT, "tests", "golden", "lookups"))
    res = {"size": S, "reps": a.reps, "rasters": 18, "storm": [P, lam], "patterns": {}}
    n_max = max(int(cell_map(S, w).max()) + 1 for w in widths)
    with gpu.Engine(0) as e:
        e.set_tables(tables)
        e.set_weights(q)
        res["device"] = e.device_info()["name"]
        acc2 = e.alloc(18 * n_max * n_max * 16)
        acc3 = e.alloc(18 * n_max * n_max * 24)
        means = e.alloc(2 * 18 * n_max * n_max)
        bytes3 = e.alloc(2 * 18 * n_max * n_max)
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
                e.grid_sums(bufs[0].ptr, S, S, bufs[3].ptr, m.ptr, m.ptr, n, n, 3, 0x1FF, acc2.ptr)

            def plain(m, n):
                e.memset(acc2.ptr, 0, 18 * n * n * 16)
                sums(m, n)
                e.grid_finish(acc2.ptr, 18, n * n, means.ptr, None, 0, None)

            def sums_weighted(m, n):
                e.grid_sums_weighted(bufs[0].ptr, S, S, bufs[3].ptr, m.ptr, m.ptr, n, n, 3, 0x1FF, acc3.ptr)

            def weighted(m, n):
                e.memset(acc3.ptr, 0, 18 * n * n * 24)
                sums_weighted(m, n)
                e.grid_finish_weighted(acc3.ptr, 18, n * n, bytes3.ptr, bytes3.at(18 * n * n), None, 0, None)

            one["copy"] = timed(e, lambda: e.stream_copy(bufs[0].ptr, copy_dst.ptr, S * S), a.reps)
            rate = 2.0 * S * S / (one["copy"]["min_ms"] * 1e-3)            # bytes read + written per second
            one["copy"]["gb_per_s"] = round(rate / 1e9, 1)
            one["read_bound_ms"] = round(S * S / rate * 1e3, 3)
            for w in widths:
                m_host = cell_map(S, w)
                n = int(m_host.max()) + 1
                m = e.upload(m_host)
                t = {"cells": n * n}
                t["mean_only"] = timed(e, lambda m=m, n=n: plain(m, n), a.reps)
                t["mean_only"]["kernel"] = timed(e, lambda m=m, n=n: sums(m, n), a.reps)
                t["weighted"] = timed(e, lambda m=m, n=n: weighted(m, n), a.reps)
                t["weighted"]["kernel"] = timed(e, lambda m=m, n=n: sums_weighted(m, n), a.reps)
                t["ratio"] = round(t["weighted"]["min_ms"] / t["mean_only"]["min_ms"], 3)
                t["kernel_ratio"] = round(t["weighted"]["kernel"]["min_ms"] / t["mean_only"]["kernel"]["min_ms"], 3)
                plain(m, n)
                weighted(m, n)
                e.sync()
                pairs = e.download(acc2.ptr, (18 * n * n, 2), np.uint64)
                triples = e.download(acc3.ptr, (18 * n * n, 3), np.uint64)
                t["words_0_1_equal"] = bool(np.array_equal(triples[:, :2], pairs))
                t["means_equal"] = bool(np.array_equal(e.download(means.ptr, (18 * n * n,)),
                                                       e.download(bytes3.ptr, (18 * n * n,))))
                cnq = e.download(bytes3.at(18 * n * n), (18 * n * n,))
                mean = e.download(bytes3.ptr, (18 * n * n,))
                wet = triples[:, 2] > 0
                t["cells_shedding_water"] = int(wet.sum())
                t["cells_above_their_mean"] = int((wet & (cnq > mean)).sum())
                t["cells_below_their_mean"] = int((wet & (cnq < mean)).sum())
                one["grid_%gpx" % w] = t
                e.sync()
                m.close()
            res["patterns"][pattern] = one
            e.sync()
            for b in bufs:
                b.close()
        for b in (acc2, acc3, means, bytes3, copy_dst):
            b.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
