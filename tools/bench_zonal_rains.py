#!/usr/bin/env python3
"""Timing of the zonal sums under several rainfall rasters (zone_rains=...): one call that counts the pixels once beside
k one-raster calls, and beside the zonal pair histogram.  One JSON line; --out also writes it to a file.

One process on one GPU, the scene of tools/bench_zonal_rain.py: a 36000 x --rows strip of the "patches" landcover, the soil
prepared once, about --zones random discs, rain cells of --cell pixels.  Every figure is the minimum and median of --reps
event-timed launches after a warm-up launch:
  (z)  gcn10_gpu_zonal_pair_histogram on the uncut spans: the yardstick, in the same run;
  (k)  gcn10_gpu_zonal_sums_rains for k = 1, 2, 4, 8 on the spans cut where any of the k layers changes;
  (1s) k calls of gcn10_gpu_zonal_sums_rain, each on its own layer's cut, timed one after the other and added.
Two families of layers: "ladder", layer j the smooth field of that tool scaled by a rising factor and clipped to a byte (the
return periods of an atlas: the layers change at the same cell edges until they clip); "iid", k independent fields, where
nearly every (zone, cell) is a piece of its own.  "ratio_to_singles" is (k) / (1s), "ratio_to_zonal" is (k) / (z).  Beside
them spans, items, the host seconds of the cutter and the bytes that come back.  Every timed variant is checked: s and n of
the new call equal those of the one-raster call on layer 0, and sw_j equals the sw of the one-raster call on layer j."""
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


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


bz = _load("bench_zonal")
bzr = _load("bench_zonal_rain")
FACTORS = [0.55, 0.7, 0.85, 1.0, 1.15, 1.3, 1.5, 1.7]       # 2 to 100 years, about


def time_rains(e, esa_ptr, W, H, cj_ptr, spans, items, n_zones, k, reps):
    bufs = [e.upload(spans), e.upload(items)]
    nbytes = n_zones * 18 * (2 + k) * 8
    acc = e.alloc(nbytes)
    e0, e1 = e.event_create(), e.event_create()
    ms = []
    try:
        for _rep in range(reps + 1):
            e.memset(acc.ptr, 0, nbytes)
            e.event_record(e0)
            e.zonal_sums_rains_device(esa_ptr, W, H, cj_ptr, bufs[0].ptr, bufs[1].ptr, items.size, n_zones, 3, 0x1FF, k,
                                      acc.ptr)
            e.event_record(e1)
            e.event_sync(e1)
            ms.append(e.elapsed_ms(e0, e1))
        words = e.download(acc.ptr, (n_zones, 18, 2 + k), np.uint64)
    finally:
        e.event_destroy(e0)
        e.event_destroy(e1)
        for b in bufs + [acc]:
            b.close()
    return ms[1:], words


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
        sp, it = host.zone_items(raw, 0, 0)
        px = int((sp["x1"] - sp["x0"]).sum())
        ms, counts = bz.time_zonal(e, bufs[0].ptr, W, H, bufs[3].ptr, sp, it, n_zones, a.reps)
        assert int(counts.sum()) == px
        z = bz.fig(ms, px)
        z.update(zones=n_zones, spans=int(sp.size), items=int(it.size), pixels=px, d2h_bytes=n_zones * bz.HIST * 8)
        res["zonal_pair_histogram"] = z

        ncx, ncy = -(-W // a.cell), -(-H // a.cell)
        gplan = {"cellx": (np.arange(W) // a.cell).astype(np.int32), "celly": (np.arange(H) // a.cell).astype(np.int32),
                 "cx0": 0, "cy0": 0}
        yy, xx = np.mgrid[0:ncy, 0:ncx]
        smooth = 20 + 60 * xx / ncx + 30 * yy / max(ncy, 1) + 6 * np.sin(xx / 9.0)
        families = {
            "ladder": np.stack([np.clip(smooth * f, 0, 255).astype(np.uint8) for f in FACTORS]),
            "iid": np.random.default_rng(3).integers(0, 256, (8, ncy, ncx)).astype(np.uint8),
        }
        for family, layers in families.items():
            # the parent's call on every layer's own cut, in this process
            singles = []
            for j in range(8):
                t0 = time.time()
                cut = host.zone_rain_cut({"spans": sp}, W, H, gplan, layers[j], n_local=n_zones)
                t_cut = time.time() - t0
                ms, triples = bzr.time_rain(e, bufs[0].ptr, W, H, bufs[3].ptr, cut["spans"], cut["items"], n_zones, a.reps)
                singles.append({"ms_min": min(ms), "ms_median": float(np.median(ms)), "spans": int(cut["spans"].size),
                                "items": int(cut["items"].size), "host_cut_seconds": t_cut, "triples": triples})
            out = {"single_ms_min": [round(s["ms_min"], 4) for s in singles],
                   "single_spans": [s["spans"] for s in singles], "single_items": [s["items"] for s in singles],
                   "single_host_cut_seconds": [round(s["host_cut_seconds"], 4) for s in singles]}
            for k in (1, 2, 4, 8):
                t0 = time.time()
                cut = host.zone_rains_cut({"spans": sp}, W, H, gplan, layers[:k], n_local=n_zones)
                t_cut = time.time() - t0
                assert int(cut["rain_pixels"].sum()) == px
                ms, words = time_rains(e, bufs[0].ptr, W, H, bufs[3].ptr, cut["spans"], cut["items"], n_zones, k, a.reps)
                assert (words[:, :, :2] == singles[0]["triples"][:, :, :2]).all()
                for j in range(k):
                    assert (words[:, :, 2 + j] == singles[j]["triples"][:, :, 2]).all(), (family, k, j)
                f = bz.fig(ms, px)
                k_singles = sum(s["ms_min"] for s in singles[:k])
                f.update(spans=int(cut["spans"].size), items=int(cut["items"].size),
                         tuples=int(len(np.unique(cut["items"]["table"], axis=0))), d2h_bytes=n_zones * 18 * (2 + k) * 8,
                         host_cut_seconds=round(t_cut, 4),
                         host_cut_seconds_of_k_singles=round(sum(s["host_cut_seconds"] for s in singles[:k]), 4),
                         k_singles_ms_min=round(k_singles, 4), d2h_bytes_of_k_singles=k * n_zones * 18 * 24,
                         ratio_to_singles=round(f["ms_min"] / k_singles, 3),
                         ratio_to_zonal=round(f["ms_min"] / z["ms_min"], 3))
                out["k%d" % k] = f
            res[family] = out
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
