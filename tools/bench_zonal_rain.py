#!/usr/bin/env python3
"""Timing of the zonal sums under a rainfall raster (zone_rain=...): the kernel beside the zonal pair histogram.  One JSON
line; --out also writes it to a file.

One process on one GPU, a 36000 x --rows strip of the "patches" landcover of bench.synth_block, the soil prepared once,
about --zones random discs that cover a third of the strip (tools/bench_zonal.py), every figure the minimum and median
of --reps event-timed launches after a warm-up launch:
  (z)  gcn10_gpu_zonal_pair_histogram on the uncut spans: the yardstick, in the same run;
  (r)  gcn10_gpu_zonal_sums_rain on the spans cut by a smooth field of 100-px cells (a plane with a ripple);
  (r') the same with an i.i.d. field: every cell edge cuts.
"ratio_to_zonal" is (r) / (z).  Beside them the host seconds of the cutter (gcn10_zone_rain_cut) and of the span builder
(gcn10_zone_items_build) for the same spans.  The triples of every timed variant are checked: n summed over the zones
is at most the pixels named, and equal for (r) and (r')."""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from gcn10_amd import gpu, host  # noqa: E402

_spec = importlib.util.spec_from_file_location("bench_zonal", os.path.join(ROOT, "tools", "bench_zonal.py"))
bz = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bz)


def time_rain(e, esa_ptr, W, H, cj_ptr, spans, items, n_zones, reps):
    bufs = [e.upload(spans), e.upload(items)]
    nbytes = n_zones * 18 * 24
    acc = e.alloc(nbytes)
    e0, e1 = e.event_create(), e.event_create()
    ms = []
    try:
        for _rep in range(reps + 1):
            e.memset(acc.ptr, 0, nbytes)
            e.event_record(e0)
            e.zonal_sums_rain_device(esa_ptr, W, H, cj_ptr, bufs[0].ptr, bufs[1].ptr, items.size, n_zones, 3, 0x1FF,
                                     acc.ptr)
            e.event_record(e1)
            e.event_sync(e1)
            ms.append(e.elapsed_ms(e0, e1))
        triples = e.download(acc.ptr, (n_zones, 18, 3), np.uint64)
    finally:
        e.event_destroy(e0)
        e.event_destroy(e1)
        for b in bufs + [acc]:
            b.close()
    return ms[1:], triples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2304)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--zones", type=int, default=1000)
    ap.add_argument("--cell", type=int, default=100, help="pixels per rain cell")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    W, H = 36000, a.rows
    res = {"W": W, "rows": H, "reps": a.reps, "cell_px": a.cell}
    with gpu.Engine(0) as e:
        res["device"] = e.device_info()
        e.set_tables(host.load_all_lookup_tables(os.path.join(ROOT, "tests", "golden", "lookups")))
        e.set_rain_tables(host.rain_tables(2.5, 0.2))
        esa, _, _, _ = bench.synth_block(1, 4096, "patches")
        esa = np.ascontiguousarray(np.tile(esa[:min(H, 4096)], ((H + 4095) // 4096, 9))[:H, :W])
        rng = np.random.default_rng(2)
        hsx, hsy = W // 25, max(H // 25, 1)
        coarse = rng.choice(bench.HSG_CODES, size=(hsy, hsx)).astype(np.uint8)
        gt = [0.0, 3.0 / W, 0.0, 3.0, 0.0, -3.0 / W]
        sgt = [0.0, 3.0 / hsx, 0.0, 3.0, 0.0, -3.0 / hsx]
        ci, cj = host.build_index_maps(gt, sgt, W, H, hsx, hsy)
        bufs = [e.upload(x) for x in (esa, coarse, ci, cj)]
        e.prepare_tile(bufs[1].ptr, hsx, hsy, bufs[2].ptr, W)

        raw, n_zones = bz.disc_spans(a.zones, W, H, np.random.default_rng(a.zones))
        raw = raw[np.lexsort((raw["x0"], raw["y"], raw["zone"]))]
        t0 = time.time()
        sp, it = host.zone_items(raw, 0, 0)
        t_items = time.time() - t0
        px = int((sp["x1"] - sp["x0"]).sum())
        ms, counts = bz.time_zonal(e, bufs[0].ptr, W, H, bufs[3].ptr, sp, it, n_zones, a.reps)
        assert int(counts.sum()) == px
        z = bz.fig(ms, px)
        z.update(zones=n_zones, spans=int(sp.size), items=int(it.size), pixels=px, d2h_bytes=n_zones * bz.HIST * 8,
                 host_items_seconds=round(t_items, 4))
        res["zonal_pair_histogram"] = z

        ncx, ncy = -(-W // a.cell), -(-H // a.cell)
        gplan = {"cellx": (np.arange(W) // a.cell).astype(np.int32), "celly": (np.arange(H) // a.cell).astype(np.int32),
                 "cx0": 0, "cy0": 0}
        yy, xx = np.mgrid[0:ncy, 0:ncx]
        smooth = np.clip(20 + 60 * xx / ncx + 30 * yy / max(ncy, 1) + 6 * np.sin(xx / 9.0), 0, 255).astype(np.uint8)
        iid = np.random.default_rng(3).integers(0, 256, (ncy, ncx)).astype(np.uint8)
        n_valid = None
        for name, field in (("rain_smooth", smooth), ("rain_iid", iid)):
            t0 = time.time()
            cut = host.zone_rain_cut({"spans": sp}, W, H, gplan, field, n_local=n_zones)
            t_cut = time.time() - t0
            assert int(cut["rain_pixels"].sum()) == px
            ms, triples = time_rain(e, bufs[0].ptr, W, H, bufs[3].ptr, cut["spans"], cut["items"], n_zones, a.reps)
            n = triples[:, :, 1].astype(np.int64)
            assert int(n.max()) <= int(cut["rain_pixels"].max()) and (n_valid is None or (n == n_valid).all())
            n_valid = n
            f = bz.fig(ms, px)
            f.update(spans=int(cut["spans"].size), items=int(cut["items"].size),
                     tables=int(len(np.unique(cut["items"]["table"]))), d2h_bytes=n_zones * 18 * 24,
                     host_cut_seconds=round(t_cut, 4), ratio_to_zonal=round(f["ms_min"] / z["ms_min"], 3))
            res[name] = f
        for b in bufs:
            b.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
