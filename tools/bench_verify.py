#!/usr/bin/env python3
"""Timing of the verification mode (DESIGN.md "Verification"), in one session:

kernel   gcn10_gpu_verify_strip over one --size^2 block of each landcover pattern, strip by strip: the 18 "file"
         rasters of a strip are made on the device by gcn10_gpu_cn_strip (not timed), the verifier's launches are
         event-timed and summed over the block.  Beside it gcn10_gpu_stream_copy over as many bytes as the verifier's
         traffic (19 x W x rows + the soil rows), the yardstick bench.py uses for the strip kernel.  Every counter must
         be zero.
program  wall seconds per block of `bin/gcn10` writing a synthetic world of --blocks blocks, and of `bin/gcn10
         --verify` over what it wrote (--no-program skips this part).

One JSON line."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from gcn10_amd import gpu, host  # noqa: E402
from tests import tiffutil  # noqa: E402

LOOKUPS = os.path.join(ROOT, "tests", "golden", "lookups")


def kernel_part(size, rows, patterns, reps):
    out = {}
    tables = host.load_all_lookup_tables(LOOKUPS)
    with gpu.Engine(0) as e:
        e.set_tables(tables)
        for pattern in patterns:
            esa, gt, coarse, sgt = bench.synth_block(1, size, pattern)
            W = H = size
            hsy, hsx = coarse.shape
            ci, cj = host.build_index_maps(gt, sgt, W, H, hsx, hsy)
            bufs = [e.upload(x) for x in (esa, coarse, ci, cj)]
            got = e.alloc(18 * W * rows)
            counts = e.verify_counts_alloc()
            e.prepare_tile(bufs[1].ptr, hsx, hsy, bufs[2].ptr, W)
            e0, e1 = e.event_create(), e.event_create()
            ptrs = [got.ptr + r * W * rows for r in range(18)]
            per_rep = []
            for _rep in range(reps + 1):
                total = 0.0
                for y0 in range(0, H, rows):
                    n = min(rows, H - y0)
                    e.cn_strip(bufs[0].ptr + y0 * W, W, n, bufs[3].ptr + 4 * y0, 3, 0x1FF, ptrs)
                    e.event_record(e0)
                    e.verify_strip(bufs[0].ptr + y0 * W, W, n, bufs[3].ptr + 4 * y0, 3, 0x1FF, ptrs, W, y0, counts.ptr)
                    e.event_record(e1)
                    e.event_sync(e1)
                    total += e.elapsed_ms(e0, e1)
                per_rep.append(total)
            c = e.verify_counts(counts.ptr)
            assert not c["mismatches"].any() and (c["first"] == gpu.VERIFY_NONE).all(), c
            # the yardstick: a plain copy that moves as many bytes (half read, half written), same run
            traffic = gpu.strip_algorithmic_bytes(W, H, hsx, hsy, 3, 0x1FF)
            nb = min(18 * W * rows // 2, traffic // 2) // 16 * 16
            copy_ms = []
            for _rep in range(reps + 1):
                e.event_record(e0)
                e.stream_copy(got.ptr, got.ptr + 9 * W * rows, nb)
                e.event_record(e1)
                e.event_sync(e1)
                copy_ms.append(e.elapsed_ms(e0, e1))
            copy_rate = 2 * nb / (min(copy_ms[1:]) * 1e-3)
            best = min(per_rep[1:])
            rate = traffic / (best * 1e-3)
            out[pattern] = {"verify_ms_per_block_min": round(best, 3),
                            "verify_ms_per_block_median": round(float(np.median(per_rep[1:])), 3),
                            "traffic_bytes": int(traffic), "verify_gb_per_s": round(rate / 1e9, 1),
                            "stream_copy_gb_per_s": round(copy_rate / 1e9, 1),
                            "fraction_of_stream_copy": round(rate / copy_rate, 3)}
            e.event_destroy(e0)
            e.event_destroy(e1)
            for b in bufs + [got, counts]:
                b.close()
    return out


def program_part(size, blocks, pattern, extra):
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        esa, _, coarse, _ = bench.synth_block(3, size, pattern)
        px = 3.0 / size
        wide = np.ascontiguousarray(np.tile(esa, (1, blocks)))
        soil = np.ascontiguousarray(np.tile(coarse, (1, blocks)))
        hs = coarse.shape[0]
        tiffutil.write_tiff(os.path.join(tmp, "esa.tif"), wide, gt=[0.0, px, 0.0, 3.0, 0.0, -px], compression=8,
                            tile=(1024, 1024), zlevel=1)
        tiffutil.write_tiff(os.path.join(tmp, "soil.tif"), soil, gt=[0.0, 3.0 / hs, 0.0, 3.0, 0.0, -3.0 / hs],
                            compression=8, tile=(256, 256))
        tiffutil.write_block_shapefile(os.path.join(tmp, "blocks"),
                                       [(i + 1, 3.0 * i, 0.0, 3.0 * (i + 1), 3.0) for i in range(blocks)])
        with open(os.path.join(tmp, "config.txt"), "w") as f:
            f.write("hysogs_data_path=%s/soil.tif\nesa_data_path=%s/esa.tif\nblocks_shp_path=%s/blocks.shp\n"
                    "lookup_table_path=%s\nlog_dir=%s/logs\n" % (tmp, tmp, tmp, LOOKUPS, tmp))
        for name, args in (("write", ["-o"]), ("verify", ["--verify"])):
            t0 = time.time()
            p = subprocess.run([os.path.join(ROOT, "bin", "gcn10"), "-c", "config.txt", "--gpus", "1"] + args + extra,
                               cwd=tmp, capture_output=True, text=True)
            wall = time.time() - t0
            res[name] = {"exit": p.returncode, "wall_s": round(wall, 3), "wall_s_per_block": round(wall / blocks, 3)}
            if name == "verify":
                said = (p.stdout + p.stderr).splitlines()
                res[name]["summary"] = [l.split("] ")[-1] for l in said if "verify: " in l][-1:]
                res[name]["findings"] = [l.split("] ")[-1][:300] for l in said
                                         if "MISMATCH" in l or "UNREADABLE" in l or "MISSING" in l][:5]
        log = open(os.path.join(tmp, "logs", "rank_0.log")).read().splitlines()
        res["timing_lines"] = [l.split("] ", 3)[-1][:400] for l in log if "timing: " in l and "blocks," in l]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=36000)
    ap.add_argument("--rows", type=int, default=2304, help="rows per strip of the kernel part")
    ap.add_argument("--patterns", default="patches,natural")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=2, help="blocks of the program part's world")
    ap.add_argument("--program-size", type=int, default=0, help="block size of the program part (0 = --size)")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--no-program", action="store_true")
    a, extra = ap.parse_known_args()
    res = {"size": a.size, "rows": a.rows}
    if not a.no_kernel:
        res["kernel"] = kernel_part(a.size, a.rows, a.patterns.split(","), a.reps)
    if not a.no_program:
        res["program"] = program_part(a.program_size or a.size, a.blocks, a.patterns.split(",")[0], extra)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
