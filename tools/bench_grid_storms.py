#!/usr/bin/env python3
"""Kernel-level timing of several design storms in one pass on a model grid (gcn10_gpu_grid_sums_storms), by the method
of tools/bench_grid_runoff.py: one process, the 36000 x 36000 blocks of bench.synth_block (patterns patches and
natural), all 18 rasters, cells of 25 px and of 1200 px:

  (m)   the mean-only trio: memset of the pairs, gcn10_gpu_grid_sums, gcn10_gpu_grid_finish;
  (w)   the weighted trio for 50 mm: memset of the triples, gcn10_gpu_grid_sums_weighted, gcn10_gpu_grid_finish_weighted;
  (s_k) memset of the 2 + k words, gcn10_gpu_grid_sums_storms, gcn10_gpu_grid_finish_storms for k = 1, 2, 4, 8 storms of
        25 ... 200 mm (k = 1: 50 mm, the work of (w)).

Every figure is the time between two events around the launches of one block, after one warm-up block; min and median
of --reps; the sums kernels alone are reported too.  Derived, from the minima of this run: s_1 / w; the cost of one more
storm (s_8 - s_1) / 7 beside w - m, what a storm costs today; s_k beside k w, the device time of k runs.  Words 0 and 1
and the means of every leg are compared with (m)'s, the 50 mm word and bytes of every (s_k) with (w)'s.  One JSON line;
--out also writes it to a file."""
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

KS = (1, 2, 4, 8)
LADDER = {1: [50], 2: [25, 50], 4: [25, 50, 75, 100], 8: [25, 50, 75, 100, 125, 150, 175, 200]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", default="patches,natural")
    ap.add_argument("--size", type=int, default=36000)
    ap.add_argument("--cells", default="25,1200", help="cell sizes in pixels")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    S = a.size
    widths = [float(c) for c in a.cells.split(",")]
    q = {p: host.runoff_table(p, 0.2) for p in LADDER[8]}
    tables = host.load_all_lookup_tables(os.path.join(ROOT, "tests", "golden", "lookups"))
    res = {"size": S, "reps": a.reps, "rasters": 18, "lambda": 0.2, "ladders_mm": {str(k): LADDER[k] for k in KS},
           "patterns": {}}
    n_max = max(int(cell_map(S, w).max()) + 1 for w in widths)
    cells_max = 18 * n_max * n_max
    with gpu.Engine(0) as e:
        e.set_tables(tables)
        res["device"] = e.device_info()["name"]
        acc2 = e.alloc(cells_max * 16)
        acc3 = e.alloc(cells_max * 24)
        acck = e.alloc(cells_max * 8 * 10)
        means = e.alloc(cells_max)
        bytes3 = e.alloc(2 * cells_max)
        bytesk = e.alloc(9 * cells_max)
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

            def sums_storms(m, n):
                e.grid_sums_storms(bufs[0].ptr, S, S, bufs[3].ptr, m.ptr, m.ptr, n, n, 3, 0x1FF, acck.ptr)

            def storms(m, n, k):
                e.memset(acck.ptr, 0, 18 * n * n * 8 * (2 + k))
                sums_storms(m, n)
                e.grid_finish_storms(acck.ptr, 18, n * n, bytesk.ptr, bytesk.at(18 * n * n), None, 0, None)

            for w in widths:
                m_host = cell_map(S, w)
                n = int(m_host.max()) + 1
                nc = 18 * n * n
                m = e.upload(m_host)
                t = {"cells": n * n}
                t["m"] = timed(e, lambda m=m, n=n: plain(m, n), a.reps)
                t["m"]["kernel"] = timed(e, lambda m=m, n=n: sums(m, n), a.reps)
                e.set_weights(q[50])
                t["w"] = timed(e, lambda m=m, n=n: weighted(m, n), a.reps)
                t["w"]["kernel"] = timed(e, lambda m=m, n=n: sums_weighted(m, n), a.reps)
                plain(m, n)
                weighted(m, n)
                e.sync()
                pairs = e.download(acc2.ptr, (nc, 2), np.uint64)
                triples = e.download(acc3.ptr, (nc, 3), np.uint64)
                mean = e.download(means.ptr, (nc,))
                cnq50 = e.download(bytes3.at(nc), (nc,))
                same = bool(np.array_equal(triples[:, :2], pairs)) and \
                    bool(np.array_equal(mean, e.download(bytes3.ptr, (nc,))))
                for k in KS:
                    e.set_weight_tables(np.stack([q[p] for p in LADDER[k]]))
                    leg = timed(e, lambda m=m, n=n, k=k: storms(m, n, k), a.reps)
                    leg["kernel"] = timed(e, lambda m=m, n=n: sums_storms(m, n), a.reps)
                    storms(m, n, k)
                    e.sync()
                    words = e.download(acck.ptr, (nc, 2 + k), np.uint64)
                    at = LADDER[k].index(50)
                    same = same and bool(np.array_equal(words[:, :2], pairs)) and \
                        bool(np.array_equal(words[:, 2 + at], triples[:, 2])) and \
                        bool(np.array_equal(e.download(bytesk.ptr, (nc,)), mean)) and \
                        bool(np.array_equal(e.download(bytesk.at((1 + at) * nc), (nc,)), cnq50))
                    t["s_%d" % k] = leg
                mn = {name: t[name]["min_ms"] for name in ["m", "w"] + ["s_%d" % k for k in KS]}
                t["words_and_bytes_equal_across_the_legs"] = same
                t["s_1_over_w"] = round(mn["s_1"] / mn["w"], 3)
                t["one_more_storm_ms"] = round((mn["s_8"] - mn["s_1"]) / 7.0, 3)
                t["a_storm_today_ms"] = round(mn["w"] - mn["m"], 3)
                t["s_k_over_k_w"] = {str(k): round(mn["s_%d" % k] / (k * mn["w"]), 3) for k in KS}
                one["grid_%gpx" % w] = t
                e.sync()
                m.close()
            res["patterns"][pattern] = one
            e.sync()
            for b in bufs:
                b.close()
        for b in (acc2, acc3, acck, means, bytes3, bytesk):
            b.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
