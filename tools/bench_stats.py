#!/usr/bin/env python3
"""Kernel-level timing of the pair histogram of the band statistics (gcn10_gpu_pair_histogram) on 36000-px strips of
each landcover pattern of bench.synth_block, in one process: the soil of the strip is prepared once
(gcn10_gpu_prepare_tile), then the histogram runs --reps times (first run dropped), each an event-timed launch.
The per-block figure scales the strip's time to 36000 rows.  One JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from gcn10_amd import gpu, host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", default="patches,natural,iid")
    ap.add_argument("--rows", type=int, default=2304, help="rows per strip (the program's default strip)")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    W, H = 36000, a.rows
    res = {"W": W, "rows": H, "target_ms_per_block": 0.5, "patterns": {}}
    with gpu.Engine(0) as e:
        for pattern in a.patterns.split(","):
            esa, _, _, _ = bench.synth_block(1, 4096, pattern)
            esa = np.ascontiguousarray(np.tile(esa[:min(H, 4096)], ((H + 4095) // 4096, 9))[:H, :W])
            rng = np.random.default_rng(2)
            hsx, hsy = W // 25, max(H // 25, 1)
            coarse = rng.choice(bench.HSG_CODES, size=(hsy, hsx)).astype(np.uint8)
            gt = [0.0, 3.0 / W, 0.0, 3.0, 0.0, -3.0 / W]
            sgt = [0.0, 3.0 / hsx, 0.0, 3.0, 0.0, -3.0 / hsx]
            ci, cj = host.build_index_maps(gt, sgt, W, H, hsx, hsy)
            bufs = [e.upload(x) for x in (esa, coarse, ci, cj)]
            hist = e.alloc(gpu.PAIR_HIST_BINS * 256 * 8)
            e.prepare_tile(bufs[1].ptr, hsx, hsy, bufs[2].ptr, W)
            e.memset(hist.ptr, 0, gpu.PAIR_HIST_BINS * 256 * 8)
            e0, e1 = e.event_create(), e.event_create()
            ms = []
            for _rep in range(a.reps + 1):
                e.event_record(e0)
                e.pair_histogram(bufs[0].ptr, W, H, bufs[3].ptr, hist.ptr)
                e.event_record(e1)
                e.event_sync(e1)
                ms.append(e.elapsed_ms(e0, e1))
            counts = e.download(hist.ptr, (gpu.PAIR_HIST_BINS * 256,), dtype=np.uint64)
            assert int(counts.sum()) == W * H * (a.reps + 1)
            best = min(ms[1:])
            res["patterns"][pattern] = {
                "ms_per_strip_min": round(best, 4), "ms_per_strip_median": round(float(np.median(ms[1:])), 4),
                "ms_per_block": round(best * 36000 / H, 3),
                "landcover_gb_per_s": round(W * H / (best * 1e-3) / 1e9, 1),
                "pairs_in_use": int((counts > 0).sum())}
            e.event_destroy(e0)
            e.event_destroy(e1)
            for b in bufs + [hist]:
                b.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
