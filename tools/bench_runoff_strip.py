#!/usr/bin/env python3
"""Kernel-level timing of the rasters of a strip through a byte table per rain cell (gcn10_gpu_runoff_strip), by the
method of tools/bench_grid_rain.py: one process on one MI355X, the 36000 x 36000 blocks of bench.synth_block (patterns
patches and natural), all 18 rasters, one call over the whole block, in the same run and on the same buffers:

  (c)    gcn10_gpu_cn_strip with 18 rasters (option compact_soil = 0: the code-bytes form the new kernel is built on; the
         default form is reported beside it as c_compact) -- the yardstick: the same 19 bytes per pixel;
  (s)    gcn10_gpu_stream_copy of the landcover: what the device streams for 1 byte in, 1 byte out;
  (r)    the new call with the 256 runoff byte tables of unit 1 mm and a constant field (cells of 100 px);
  (r')   the same with a smooth field and with an i.i.d. field of 100-px cells;
  (r'')  an i.i.d. field of 16-px cells.

Every figure is the time between two events around the call (for the new call: the expansion pre-kernel and the strip
kernel), after one warm-up call; min and median of --reps.  "kernel" is the strip kernel alone, from the events
gcn10_gpu_time_next_strip attaches to its dispatch.  The output bytes of every timed variant are compared with numpy on
sampled rows -- the oracle's curve numbers of those rows through the tables -- before a number is accepted.  Derived, from
the minima: r / c, r' / r, r'' / r.  One JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from gcn10_amd import gpu, host  # noqa: E402
from oracle import cn_oracle_c as oc  # noqa: E402
from tools.bench_grid import cell_map, timed  # noqa: E402

RESOURCES = {   # hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage (profiles/runoff_strip/resource_usage.txt)
    "runoff_strip_kernel<256>": {"vgprs": 114, "agprs": 0, "sgprs": 106, "scratch_bytes": 0, "waves_per_simd": 4,
                                 "lds_bytes": "24672 + (k + 1) * 260, dynamic"},
    "runoff_strip_kernel<1024>": {"vgprs": 114, "agprs": 0, "sgprs": 106, "scratch_bytes": 0, "waves_per_simd": 4,
                                  "lds_bytes": "24672 + (k + 1) * 260, dynamic (k = 256: 91492)"},
}


def kernel_ms(e, fn, reps):
    """the strip kernel alone: events attached to its dispatch"""
    e0, e1 = e.event_create(), e.event_create()
    ms = []
    for _rep in range(reps + 1):
        e.time_next_strip(e0, e1)
        fn()
        e.event_sync(e1)
        ms.append(e.elapsed_ms(e0, e1))
    e.event_destroy(e0)
    e.event_destroy(e1)
    return {"min_ms": round(min(ms[1:]), 3), "median_ms": round(float(np.median(ms[1:])), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", default="patches,natural")
    ap.add_argument("--size", type=int, default=36000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", default="0,1,17,4999,18000,35999", help="the rows compared with numpy")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    S = a.size
    assert a.reps >= 5, "at least 5 launches"
    rows = sorted({min(int(y), S - 1) for y in a.rows.split(",")})
    tables = host.load_all_lookup_tables(os.path.join(ROOT, "tests", "golden", "lookups"))
    T = host.runoff_bytes(host.rain_tables(1.0, 0.2), 100)
    ident = np.tile(np.arange(256, dtype=np.uint8), (256, 1))
    res = {"size": S, "reps": a.reps, "rasters": 18, "k": 256, "unit_mm": 1.0, "lambda": 0.2, "rows_checked": rows,
           "resources": RESOURCES, "patterns": {}}
    rng = np.random.default_rng(7)
    fields = {}
    for name, w in (("constant", 100.0), ("smooth", 100.0), ("iid", 100.0), ("iid_16px", 16.0)):
        m = cell_map(S, w)
        n = int(m.max()) + 1
        if name == "constant":
            f = np.full((n, n), 50, np.uint8)
        elif name == "smooth":
            yy, xx = np.mgrid[0:n, 0:n]
            f = (127.5 + 127.5 * np.sin(xx / 23.0) * np.cos(yy / 31.0)).astype(np.uint8)
        else:
            f = rng.integers(0, 256, (n, n)).astype(np.uint8)
        fields[name] = (m, n, f)
    with gpu.Engine(0) as e:
        e.set_tables(tables)
        e.set_cell_byte_tables(T)
        res["device"] = e.device_info()["name"]
        outs = [e.alloc(S * S) for _r in range(18)]
        ptrs = [o.ptr for o in outs]
        copy = e.alloc(S * S)
        for pattern in a.patterns.split(","):
            esa, gt, coarse, sgt = bench.synth_block(1, S, pattern)
            hsy, hsx = coarse.shape
            ci, cj = host.build_index_maps(gt, sgt, S, S, hsx, hsy)
            # the oracle's curve numbers of the sampled rows
            cn = {}
            for y in rows:
                soil = coarse[cj[y]][np.where(ci.view(np.uint32) < hsx, ci, hsx - 1)].reshape(1, S)
                for c in range(2):
                    hsg = oc.modify_hysogs_data(soil, c == 0)
                    for k in range(9):
                        cn[(y, c * 9 + k)] = oc.calculate_cn(esa[y:y + 1], hsg, tables[k]).reshape(S)
            bufs = [e.upload(x) for x in (esa, coarse, ci, cj)]
            del esa
            e.prepare_tile(bufs[1].ptr, hsx, hsy, bufs[2].ptr, S)

            def check(want_of):
                e.sync()
                for y in rows:
                    for r in range(18):
                        got = e.download(outs[r].at(y * S), (S,))
                        if not np.array_equal(got, want_of(y, r)):
                            raise SystemExit("%s: raster %d row %d differs from numpy" % (pattern, r, y))
                return True

            def cn_strip():
                e.cn_strip(bufs[0].ptr, S, S, bufs[3].ptr, 3, 0x1FF, ptrs)

            one = {"s": timed(e, lambda: e.stream_copy(bufs[0].ptr, copy.ptr, S * S), a.reps)}
            one["c_compact"] = timed(e, cn_strip, a.reps)
            one["c_compact"]["kernel_name"] = e.last_kernel_name()
            e.set_option("compact_soil", 0)
            one["c"] = timed(e, cn_strip, a.reps)
            one["c"]["kernel_name"] = e.last_kernel_name()
            one["c"]["rows_equal_numpy"] = check(lambda y, r: cn[(y, r)])
            e.set_option("compact_soil", 1)
            for name, (m, n, f) in fields.items():
                dm, df = e.upload(m), e.upload(f)

                def runoff():
                    e.runoff_strip(bufs[0].ptr, S, S, bufs[3].ptr, dm.ptr, dm.ptr, n, n, df.ptr, 3, 0x1FF, ptrs)

                t = timed(e, runoff, a.reps)
                t["kernel"] = kernel_ms(e, runoff, a.reps)
                t["kernel_name"] = e.last_kernel_name()
                t["cells"] = n * n
                t["rows_equal_numpy"] = check(lambda y, r: T[f[m[y]][m], cn[(y, r)]])
                one["r_" + name] = t
                e.sync()
                dm.close()
                df.close()
            # the identity tables: the new call writes cn_strip's bytes
            e.set_cell_byte_tables(ident)
            m, n, f = fields["iid"]
            dm, df = e.upload(m), e.upload(f)
            e.runoff_strip(bufs[0].ptr, S, S, bufs[3].ptr, dm.ptr, dm.ptr, n, n, df.ptr, 3, 0x1FF, ptrs)
            one["identity_rows_equal_numpy"] = check(lambda y, r: cn[(y, r)])
            e.set_cell_byte_tables(T)
            dm.close()
            df.close()
            r0 = one["r_constant"]["min_ms"]
            one["r_over_c"] = round(r0 / one["c"]["min_ms"], 3)
            one["r_over_c_compact"] = round(r0 / one["c_compact"]["min_ms"], 3)
            one["r_kernel_over_c"] = round(one["r_constant"]["kernel"]["min_ms"] / one["c"]["min_ms"], 3)
            one["r_smooth_over_r"] = round(one["r_smooth"]["min_ms"] / r0, 3)
            one["r_iid_over_r"] = round(one["r_iid"]["min_ms"] / r0, 3)
            one["r_iid_16px_over_r"] = round(one["r_iid_16px"]["min_ms"] / r0, 3)
            one["c_over_s"] = round(one["c"]["min_ms"] / one["s"]["min_ms"], 3)
            res["patterns"][pattern] = one
            e.sync()
            for b in bufs:
                b.close()
        for b in outs + [copy]:
            b.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
