#!/usr/bin/env python3
"""Kernel-level timing of the LZW tile encoder (gcn10_gpu_lzw_strip) against the per-raster DEFLATE encoder
(gcn10_gpu_deflate_strip) on the same 18 CN strips, in one process: the strips are made on the GPU
(gcn10_gpu_cn_strip) from a strip of a 36000-px block of each landcover pattern (those of tools/bench_fused.py),
then each encoder runs --reps times (first run dropped).  Event-timed launch sequences; one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from gcn10_amd import gpu, host  # noqa: E402
LOOKUPS = os.path.join(ROOT, "tests", "golden", "lookups")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", default="patches,natural")
    ap.add_argument("--rows", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    W, H, n = 36000, a.rows, 18
    across, down = (W + 255) // 256, (H + 255) // 256
    tabs = host.load_all_lookup_tables(LOOKUPS)
    res = {"W": W, "rows": H, "rasters": n, "patterns": {}}
    with gpu.Engine(0) as e:
        e.set_tables(tabs)
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
            outs = [e.alloc(W * H) for _ in range(n)]
            e.prepare_tile(bufs[1].ptr, hsx, hsy, bufs[2].ptr, W)
            e.cn_strip(bufs[0].ptr, W, H, bufs[3].ptr, 3, 0x1FF, [o.ptr for o in outs])
            ptrs = e.upload(np.array([o.ptr for o in outs], np.uint64))
            cap = max(int(gpu.lib().gcn10_gpu_lzw_arena_bound(W, H, n)), int(gpu.lib().gcn10_gpu_deflate_arena_bound(W, H, n)))
            arena, table, cursor = e.alloc(cap), e.alloc(n * across * down * 8), e.alloc(8)
            e0, e1 = e.event_create(), e.event_create()
            r = {}
            for name, fn in (("deflate", gpu.lib().gcn10_gpu_deflate_strip), ("lzw", gpu.lib().gcn10_gpu_lzw_strip)):
                ms = []
                for rep in range(a.reps + 1):
                    e.event_record(e0)
                    e._chk(fn(e._ctx, ptrs.ptr, n, W, H, arena.ptr, cap, table.ptr, cursor.ptr, None), name)
                    e.event_record(e1)
                    e.event_sync(e1)
                    ms.append(e.elapsed_ms(e0, e1))
                tab = e.download(table.ptr, (n * across * down, 2), dtype=np.uint32)
                assert (tab[:, 0] != 0xFFFFFFFF).all()
                r[name] = {"ms_min": round(min(ms[1:]), 3), "ms_median": round(float(np.median(ms[1:])), 3),
                           "stream_bytes": int(tab[:, 1].astype(np.int64).sum()),
                           "arena_bytes": int(e.download(cursor.ptr, (1,), dtype=np.uint64)[0])}
            r["lzw_over_deflate_time"] = round(r["lzw"]["ms_min"] / r["deflate"]["ms_min"], 2)
            r["lzw_over_deflate_bytes"] = round(r["lzw"]["stream_bytes"] / r["deflate"]["stream_bytes"], 3)
            res["patterns"][pattern] = r
            e.event_destroy(e0)
            e.event_destroy(e1)
            for b in bufs + outs + [ptrs, arena, table, cursor]:
                b.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
