#!/usr/bin/env python3
"""Timing of the zonal composites (zonal=1): the kernel alone, and the program end to end.  One JSON line each.

Kernel (default): one process on one GPU, 36000 x --rows strips of each landcover pattern of bench.synth_block, the
soil prepared once, every figure the minimum and median of --reps event-timed launches after a warm-up launch:
  (c) gcn10_gpu_pair_histogram on the strip: the yardstick;
  (a) gcn10_gpu_zonal_pair_histogram with ONE zone covering the strip, for every (span, item) bound of --bounds:
      the same pixels as (c) plus the span bookkeeping; "ratio_to_pair_histogram" is (a) / (c);
  (b) the same kernel with about 1 000 and about 100 000 random small zones (discs) that cover about a third of it.
The counts of every timed variant are checked against the pixels its spans name.

--pipeline: bin/gcn10 --zones on --blocks x --repeat patchy 36000^2 blocks (the world of tools/bench_pipeline.py) with
--zones-n random polygons, against the default write run with GCN10_SINK=null in the same session: steady-state
seconds per block of both, and the host seconds per block spent building spans."""
import argparse
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from gcn10_amd import gpu, host, shapefile  # noqa: E402

HIST = gpu.PAIR_HIST_BINS * 256


def disc_spans(n_zones, W, H, rng, cover=0.33):
    """about n_zones random discs (clipped to the strip) whose areas add up to `cover` of it, as sorted spans"""
    r0 = max(1.0, np.sqrt(cover * W * H / n_zones / np.pi))
    cx, cy = rng.uniform(0, W, n_zones), rng.uniform(0, H, n_zones)
    rad = rng.uniform(0.5 * r0, 1.4 * r0, n_zones)
    rmax = int(np.ceil(rad.max()))
    dy = np.arange(-rmax, rmax + 1)
    y = np.floor(cy)[:, None] + dy[None, :]                                  # [zone][row]
    half2 = rad[:, None] ** 2 - (y + 0.5 - cy[:, None]) ** 2
    ok = (half2 > 0) & (y >= 0) & (y < H)
    half = np.sqrt(np.where(ok, half2, 0.0))
    x0 = np.clip(np.ceil(cx[:, None] - half - 0.5), 0, W).astype(np.int64)
    x1 = np.clip(np.ceil(cx[:, None] + half - 0.5), 0, W).astype(np.int64)
    ok &= x0 < x1
    zone = np.repeat(np.arange(n_zones)[:, None], dy.size, axis=1)
    sp = np.zeros(int(ok.sum()), host.ZONE_SPAN_DTYPE)
    sp["y"], sp["x0"], sp["x1"] = y[ok], x0[ok], x1[ok]
    # zones without a pixel in the strip get no index: local zones are dense
    _u, dense = np.unique(zone[ok], return_inverse=True)
    sp["zone"] = dense
    return sp, int(dense.max()) + 1 if sp.size else 0


def time_zonal(e, esa_ptr, W, H, cj_ptr, spans, items, n_zones, reps):
    """event-timed launches over uploaded spans and items; returns (ms list, counts of the last launch per zone)"""
    bufs = [e.upload(spans), e.upload(items)]
    hist = e.alloc(n_zones * HIST * 8)
    e0, e1 = e.event_create(), e.event_create()
    ms = []
    try:
        for _rep in range(reps + 1):
            e.memset(hist.ptr, 0, n_zones * HIST * 8)
            e.event_record(e0)
            e.zonal_pair_histogram_device(esa_ptr, W, H, cj_ptr, bufs[0].ptr, bufs[1].ptr, items.size, n_zones, hist.ptr)
            e.event_record(e1)
            e.event_sync(e1)
            ms.append(e.elapsed_ms(e0, e1))
        counts = e.download(hist.ptr, (n_zones, HIST), np.uint64).sum(axis=1)
    finally:
        e.event_destroy(e0)
        e.event_destroy(e1)
        for b in bufs + [hist]:
            b.close()
    return ms[1:], counts


def fig(ms, px):
    best = min(ms)
    return {"ms_min": round(best, 4), "ms_median": round(float(np.median(ms)), 4), "gpx_per_s": round(px / best / 1e6, 1)}


def kernel_bench(a):
    W, H = 36000, a.rows
    bounds = [tuple(int(v) for v in b.split(":")) for b in a.bounds.split(",")]
    res = {"W": W, "rows": H, "reps": a.reps, "patterns": {}}
    with gpu.Engine(0) as e:
        res["device"] = e.device_info()
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
            e.prepare_tile(bufs[1].ptr, hsx, hsy, bufs[2].ptr, W)
            out = {}
            # (c) the yardstick
            hist = e.alloc(HIST * 8)
            e.memset(hist.ptr, 0, HIST * 8)
            e0, e1 = e.event_create(), e.event_create()
            ms = []
            for _rep in range(a.reps + 1):
                e.event_record(e0)
                e.pair_histogram(bufs[0].ptr, W, H, bufs[3].ptr, hist.ptr)
                e.event_record(e1)
                e.event_sync(e1)
                ms.append(e.elapsed_ms(e0, e1))
            assert int(e.download(hist.ptr, (HIST,), np.uint64).sum()) == W * H * (a.reps + 1)
            hist.close()
            e.event_destroy(e0)
            e.event_destroy(e1)
            out["pair_histogram"] = fig(ms[1:], W * H)
            # (a) one zone over the strip, per bound
            whole = np.zeros(H, host.ZONE_SPAN_DTYPE)
            whole["y"], whole["x1"] = np.arange(H), W
            out["one_zone"] = {}
            for span_px, item_px in bounds:
                sp, it = host.zone_items(whole, span_px, item_px)
                ms, counts = time_zonal(e, bufs[0].ptr, W, H, bufs[3].ptr, sp, it, 1, a.reps)
                assert int(counts[0]) == W * H
                f = fig(ms, W * H)
                f.update(spans=int(sp.size), items=int(it.size),
                         ratio_to_pair_histogram=round(f["ms_min"] / out["pair_histogram"]["ms_min"], 3))
                out["one_zone"]["%d:%d" % (span_px, item_px)] = f
            # (b) many small zones
            out["small_zones"] = {}
            for n in (1000, 100000):
                raw, n_zones = disc_spans(n, W, H, np.random.default_rng(n))
                raw = raw[np.lexsort((raw["x0"], raw["y"], raw["zone"]))]
                t0 = time.time()
                sp, it = host.zone_items(raw, 0, 0)
                t_items = time.time() - t0
                px = int((sp["x1"] - sp["x0"]).sum())
                ms, counts = time_zonal(e, bufs[0].ptr, W, H, bufs[3].ptr, sp, it, n_zones, a.reps)
                assert int(counts.sum()) == px
                f = fig(ms, px)
                f.update(zones=n_zones, spans=int(sp.size), items=int(it.size), pixels=px,
                         hist_MiB=round(n_zones * HIST * 8 / 2**20, 1), host_items_seconds=round(t_items, 4))
                out["small_zones"][str(n)] = f
            res["patterns"][pattern] = out
            for b in bufs:
                b.close()
    print(json.dumps(res))


def random_polygons(n, x0, y0, x1, y1, rng, vertices=16):
    """n star-shaped polygons inside the box, about a quarter of its area in all"""
    r0 = np.sqrt(0.25 * (x1 - x0) * (y1 - y0) / n / np.pi)
    zones = []
    for i in range(n):
        cx, cy = rng.uniform(x0, x1), rng.uniform(y0, y1)
        ang = np.sort(rng.uniform(0, 2 * np.pi, vertices))
        rad = rng.uniform(0.5 * r0, 1.5 * r0, vertices)
        zones.append((i + 1, [list(zip((cx + rad * np.cos(ang)).tolist(), (cy + rad * np.sin(ang)).tolist()))]))
    return zones


def pipeline_bench(a):
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_pipeline", os.path.join(ROOT, "tools", "bench_pipeline.py"))
    bp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bp)
    # a directory of this run's own, made here and removed at the end: nothing that was there before is touched
    os.makedirs(a.workdir, exist_ok=True)
    wd, size, nb = tempfile.mkdtemp(prefix="gcn10_zonal_bench_", dir=a.workdir), 36000, a.blocks
    t0 = time.time()
    bp.build_world(types.SimpleNamespace(pattern="patches", esa_compression=8, esa_predictor=1, dual_soil_fraction=-1.0,
                                         repeat=a.repeat), wd, size, nb, 3.0 / size)
    shapefile.write_zone_shapefile(os.path.join(wd, "zones"),
                                  random_polygons(a.zones_n, 0.0, 0.0, 3.0 * nb, 3.0, np.random.default_rng(5)))
    with open(os.path.join(wd, "config.txt"), "w") as f:
        f.write("hysogs_data_path=%s/soil.tif\nesa_data_path=%s/esa.tif\nblocks_shp_path=%s/blocks.shp\n"
                "lookup_table_path=%s\nlog_dir=%s/logs\n" % (wd, wd, wd, os.path.join(ROOT, "tests", "golden", "lookups"), wd))
    res = {"size": size, "blocks": nb * a.repeat, "zones": a.zones_n, "world_build_seconds": round(time.time() - t0, 1),
           "modes": {}}
    print("world built in %.0f s" % (time.time() - t0), file=sys.stderr, flush=True)
    for mode, args, env in (("zonal", ["--zones", "zones.shp"], {}), ("write_null_sink", ["-o"], {"GCN10_SINK": "null"}),
                            ("zonal_again", ["--zones", "zones.shp"], {})):
        shutil.rmtree(os.path.join(wd, "logs"), ignore_errors=True)
        t0 = time.time()
        out = subprocess.run([os.path.join(ROOT, "bin", "gcn10"), "-c", "config.txt", "--gpus", "1"] + args, cwd=wd,
                             env=dict(os.environ, **env), capture_output=True, text=True)
        wall = time.time() - t0
        p = os.path.join(wd, "logs", "rank_0.log")
        log = open(p).read() if os.path.exists(p) else ""
        ms = re.search(r"timing: steady state ([0-9.]+) s per block", log)
        mz = re.search(r"timing: zonal: host seconds building spans ([0-9.]+) \(([0-9.]+) per block.*adding histograms up ([0-9.]+)", log)
        mc = re.search(r"zonal: (\d+) blocks, (\d+) zones, (\d+) without pixels", log)
        mp = re.search(r"pinned host memory allocated ([0-9.]+) MB; peak resident set ([0-9.]+) MB", log)
        res["modes"][mode] = {"rc": out.returncode, "wall_seconds": round(wall, 2),
                              "steady_seconds_per_block": float(ms.group(1)) if ms else None,
                              "span_building_seconds_per_block": float(mz.group(2)) if mz else None,
                              "adding_up_seconds": float(mz.group(3)) if mz else None,
                              "closing_line": mc.group(0) if mc else None,
                              "pinned_MB": float(mp.group(1)) if mp else None,
                              "stderr_tail": out.stderr[-300:] if out.returncode else ""}
        print("%s: rc %d in %.0f s" % (mode, out.returncode, wall), file=sys.stderr, flush=True)
    print(json.dumps(res))
    shutil.rmtree(wd, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", default="patches,natural")
    ap.add_argument("--rows", type=int, default=2304, help="rows per strip")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--bounds", default="0:0,1024:16384,4096:16384,4096:262144,16384:65536,36000:288000",
                    help="max_span_px:max_item_px pairs of the one-zone figure (0:0 = the built-in bounds)")
    ap.add_argument("--pipeline", action="store_true", help="the program end to end instead of the kernel")
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=6)
    ap.add_argument("--zones-n", type=int, default=3000)
    ap.add_argument("--workdir", default=tempfile.gettempdir(), help="where --pipeline makes (and removes) its directory")
    a = ap.parse_args()
    (pipeline_bench if a.pipeline else kernel_bench)(a)


if __name__ == "__main__":
    main()
