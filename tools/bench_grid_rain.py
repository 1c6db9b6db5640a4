#!/usr/bin/env python3
"""Kernel-level timing of the sums on a model grid with a weight table per cell (gcn10_gpu_grid_sums_rain), by the
method of tools/bench_grid_storms.py: one process, the 36000 x 36000 blocks of bench.synth_block (patterns patches and
natural), all 18 rasters, cells of 25 px, 120 px and 1200 px:

  (w)   the weighted trio for 50 mm: memset of the triples, gcn10_gpu_grid_sums_weighted, gcn10_gpu_grid_finish_weighted
        -- unchanged code, the yardstick;
  (r)   memset + gcn10_gpu_grid_sums_rain + gcn10_gpu_grid_finish_rain with the 256 tables of unit 1 mm and a constant
        field of 50;
  (r')  the same with a random field;
  (h)   gcn10_gpu_pair_histogram over the same pixels, the floor of a kernel that counts pairs;
  (c)   a plain copy of the landcover.

Every figure is the time between two events around the launches of one block, after one warm-up block; min and median
of --reps; the sums kernels alone are reported too.  Derived, from the minima of this run: r / w, r' / r (the cost of
distinct tables) and the rain kernel alone over (h).  (r)'s triples and bytes are compared with (w)'s.  One JSON line;
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
    tables = host.load_all_lookup_tables(os.path.join(ROOT, "tests", "golden", "lookups"))
    q = host.rain_tables(1.0, 0.2)
    assert np.array_equal(q[50], host.runoff_table(50, 0.2))
    cols, rows = gpu.grid_rain_item()
    res = {"size": S, "reps": a.reps, "rasters": 18, "lambda": 0.2, "unit_mm": 1.0, "item": [cols, rows], "patterns": {}}
    n_max = max(int(cell_map(S, w).max()) + 1 for w in widths)
    cells_max = 18 * n_max * n_max
    with gpu.Engine(0) as e:
        e.set_tables(tables)
        e.set_weights(q[50])
        e.set_rain_tables(q)
        res["device"] = e.device_info()["name"]
        acc_w = e.alloc(cells_max * 24)
        acc_r = e.alloc(cells_max * 24)
        bytes_w = e.alloc(2 * cells_max)
        bytes_r = e.alloc(2 * cells_max)
        hist = e.alloc(gpu.PAIR_HIST_BINS * 256 * 8)
        copy = e.alloc(S * S)
        for pattern in a.patterns.split(","):
            esa, gt, coarse, sgt = bench.synth_block(1, S, pattern)
            hsy, hsx = coarse.shape
            ci, cj = host.build_index_maps(gt, sgt, S, S, hsx, hsy)
            bufs = [e.upload(x) for x in (esa, coarse, ci, cj)]
            del esa
            e.prepare_tile(bufs[1].ptr, hsx, hsy, bufs[2].ptr, S)
            one = {"copy": timed(e, lambda: e.stream_copy(bufs[0].ptr, copy.ptr, S * S), a.reps)}

            def histogram():
                e.pair_histogram(bufs[0].ptr, S, S, bufs[3].ptr, hist.ptr)

            one["h"] = timed(e, histogram, a.reps)

            def sums_weighted(m, n):
                e.grid_sums_weighted(bufs[0].ptr, S, S, bufs[3].ptr, m.ptr, m.ptr, n, n, 3, 0x1FF, acc_w.ptr)

            def weighted(m, n):
                e.memset(acc_w.ptr, 0, 18 * n * n * 24)
                sums_weighted(m, n)
                e.grid_finish_weighted(acc_w.ptr, 18, n * n, bytes_w.ptr, bytes_w.at(18 * n * n), None, 0, None)

            def sums_rain(m, n, f):
                e.grid_sums_rain(bufs[0].ptr, S, S, bufs[3].ptr, m.ptr, m.ptr, n, n, 3, 0x1FF, f.ptr, acc_r.ptr)

            def rain(m, n, f):
                e.memset(acc_r.ptr, 0, 18 * n * n * 24)
                sums_rain(m, n, f)
                e.grid_finish_rain(acc_r.ptr, 18, n * n, f.ptr, bytes_r.ptr, bytes_r.at(18 * n * n), None, 0, None)

            for w in widths:
                m_host = cell_map(S, w)
                n = int(m_host.max()) + 1
                nc = 18 * n * n
                m = e.upload(m_host)
                fifty = e.upload(np.full(n * n, 50, np.uint8))
                mixed = e.upload(np.random.default_rng(7).integers(0, 256, n * n).astype(np.uint8))
                t = {"cells": n * n}
                t["w"] = timed(e, lambda: weighted(m, n), a.reps)
                t["w"]["kernel"] = timed(e, lambda: sums_weighted(m, n), a.reps)
                t["r"] = timed(e, lambda: rain(m, n, fifty), a.reps)
                t["r"]["kernel"] = timed(e, lambda: sums_rain(m, n, fifty), a.reps)
                t["r_random"] = timed(e, lambda: rain(m, n, mixed), a.reps)
                t["r_random"]["kernel"] = timed(e, lambda: sums_rain(m, n, mixed), a.reps)
                weighted(m, n)
                rain(m, n, fifty)
                e.sync()
                t["triples_and_bytes_of_r_equal_w"] = \
                    bool(np.array_equal(e.download(acc_r.ptr, (nc, 3), np.uint64), e.download(acc_w.ptr, (nc, 3), np.uint64))) \
                    and bool(np.array_equal(e.download(bytes_r.ptr, (2 * nc,)), e.download(bytes_w.ptr, (2 * nc,))))
                t["r_over_w"] = round(t["r"]["min_ms"] / t["w"]["min_ms"], 3)
                t["r_random_over_r"] = round(t["r_random"]["min_ms"] / t["r"]["min_ms"], 3)
                t["r_kernel_over_h"] = round(t["r"]["kernel"]["min_ms"] / one["h"]["min_ms"], 3)
                t["r_kernel_over_w_kernel"] = round(t["r"]["kernel"]["min_ms"] / t["w"]["kernel"]["min_ms"], 3)
                one["grid_%gpx" % w] = t
                e.sync()
                for b in (m, fifty, mixed):
                    b.close()
            res["patterns"][pattern] = one
            e.sync()
            for b in bufs:
                b.close()
        for b in (acc_w, acc_r, bytes_w, bytes_r, hist, copy):
            b.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
