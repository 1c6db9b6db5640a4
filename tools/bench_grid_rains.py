#!/usr/bin/env python3
"""Kernel-level timing of the sums on a model grid with k weight tables per cell, counted once
(gcn10_gpu_grid_sums_rains), by the method of tools/bench_grid_rain.py: one process, the 36000 x 36000 blocks of
bench.synth_block (patterns patches and natural), all 18 rasters, cells of 25 px, 120 px and 1200 px, the 256 tables of
unit 1 mm, independent random fields:

  (r1)  memset of the triples, gcn10_gpu_grid_sums_rain, gcn10_gpu_grid_finish_rain -- unchanged code, the yardstick;
  (rk)  memset of the 2 + k words, gcn10_gpu_grid_sums_rains, gcn10_gpu_grid_finish_rains for k = 1, 2, 4 and 8, layer 0
        the field of (r1).

Every figure is the time between two events around the launches of one block, after one warm-up block; min and median
of --reps, so that the spread of a figure shows; the sums kernels alone are reported too.  Derived, from the minima of
this run: (rk for k = 1) / (r1); the cost of one more layer, (r8 - r1) / 7, in ms; and (r8) / (8 x r1).  The words and
bytes of k = 1 are compared with (r1)'s, and layer 0 of k = 8 with them too.  One JSON line; --out also writes it to a
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
from tools.bench_grid import cell_map, timed  # noqa: E402

LAYERS = (1, 2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", default="patches,natural")
    ap.add_argument("--size", type=int, default=36000)
    ap.add_argument("--cells", default="25,120,1200", help="cell sizes in pixels")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    S = a.size
    widths = [float(c) for c in a.cells.split(",")]
    k_max = max(LAYERS)
    tables = host.load_all_lookup_tables(os.path.join(ROOT, "tests", "golden", "lookups"))
    q = host.rain_tables(1.0, 0.2)
    cols, rows = gpu.grid_rain_item()
    res = {"size": S, "reps": a.reps, "rasters": 18, "lambda": 0.2, "unit_mm": 1.0, "item": [cols, rows],
           "layers": list(LAYERS), "patterns": {}}
    n_max = max(int(cell_map(S, w).max()) + 1 for w in widths)
    cells_max = 18 * n_max * n_max
    with gpu.Engine(0) as e:
        e.set_tables(tables)
        e.set_rain_tables(q)
        res["device"] = e.device_info()["name"]
        acc_1 = e.alloc(cells_max * 24)
        acc_k = e.alloc(cells_max * 8 * (2 + k_max))
        bytes_1 = e.alloc(2 * cells_max)
        bytes_k = e.alloc((1 + k_max) * cells_max)
        for pattern in a.patterns.split(","):
            esa, gt, coarse, sgt = bench.synth_block(1, S, pattern)
            hsy, hsx = coarse.shape
            ci, cj = host.build_index_maps(gt, sgt, S, S, hsx, hsy)
            bufs = [e.upload(x) for x in (esa, coarse, ci, cj)]
            del esa
            e.prepare_tile(bufs[1].ptr, hsx, hsy, bufs[2].ptr, S)
            one = {}

            def sums_rain(m, n, f):
                e.grid_sums_rain(bufs[0].ptr, S, S, bufs[3].ptr, m.ptr, m.ptr, n, n, 3, 0x1FF, f.ptr, acc_1.ptr)

            def rain(m, n, f):
                e.memset(acc_1.ptr, 0, 18 * n * n * 24)
                sums_rain(m, n, f)
                e.grid_finish_rain(acc_1.ptr, 18, n * n, f.ptr, bytes_1.ptr, bytes_1.at(18 * n * n), None, 0, None)

            def sums_rains(m, n, f, k):
                e.grid_sums_rains(bufs[0].ptr, S, S, bufs[3].ptr, m.ptr, m.ptr, n, n, 3, 0x1FF, f.ptr, k, acc_k.ptr)

            def rains(m, n, f, k):
                e.memset(acc_k.ptr, 0, 18 * n * n * 8 * (2 + k))
                sums_rains(m, n, f, k)
                e.grid_finish_rains(acc_k.ptr, 18, n * n, f.ptr, k, bytes_k.ptr, bytes_k.at(18 * n * n), None, 0, None)

            for w in widths:
                m_host = cell_map(S, w)
                n = int(m_host.max()) + 1
                nc = 18 * n * n
                m = e.upload(m_host)
                # independent fields, layer by layer; the _rain pair takes layer 0
                f = e.upload(np.random.default_rng(7).integers(0, 256, (k_max, n * n)).astype(np.uint8))
                t = {"cells": n * n}
                t["r1"] = timed(e, lambda: rain(m, n, f), a.reps)
                t["r1"]["kernel"] = timed(e, lambda: sums_rain(m, n, f), a.reps)
                for k in LAYERS:
                    t["r_k%d" % k] = timed(e, lambda: rains(m, n, f, k), a.reps)
                    t["r_k%d" % k]["kernel"] = timed(e, lambda: sums_rains(m, n, f, k), a.reps)
                rain(m, n, f)
                rains(m, n, f, 1)
                e.sync()
                words_1 = e.download(acc_1.ptr, (nc, 3), np.uint64)
                t["words_and_bytes_of_k1_equal_r1"] = \
                    bool(np.array_equal(e.download(acc_k.ptr, (nc, 3), np.uint64), words_1)) \
                    and bool(np.array_equal(e.download(bytes_k.ptr, (2 * nc,)), e.download(bytes_1.ptr, (2 * nc,))))
                rains(m, n, f, k_max)
                e.sync()
                t["layer_0_of_k%d_equals_r1" % k_max] = \
                    bool(np.array_equal(e.download(acc_k.ptr, (nc, 2 + k_max), np.uint64)[:, :3], words_1)) \
                    and bool(np.array_equal(e.download(bytes_k.ptr, (2 * nc,)), e.download(bytes_1.ptr, (2 * nc,))))
                del words_1
                r1, r8 = t["r1"]["min_ms"], t["r_k%d" % k_max]["min_ms"]
                t["k1_over_r1"] = round(t["r_k1"]["min_ms"] / r1, 3)
                t["ms_per_further_layer"] = round((r8 - r1) / (k_max - 1), 3)
                t["r%d_over_%d_r1" % (k_max, k_max)] = round(r8 / (k_max * r1), 3)
                one["grid_%gpx" % w] = t
                e.sync()
                for b in (m, f):
                    b.close()
            res["patterns"][pattern] = one
            e.sync()
            for b in bufs:
                b.close()
        for b in (acc_1, acc_k, bytes_1, bytes_k):
            b.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
