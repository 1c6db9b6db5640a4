#!/usr/bin/env python3
"""What profiles/column_lanes/README.md quotes, from the raw outputs of one visit.

  summarize.py bench DIR        medians, minima, maxima and ranges of bench_{parent,new}_N.json in DIR
  summarize.py pairs TRACE.csv  a rocprofv3 --kernel-trace CSV of `bench.py --no-cpu-baseline --no-also`: medians of
                                the prepare kernel, the gap to the strip kernel and the strip kernel, last 20 pairs
  summarize.py traffic FETCH.csv FETCH.json WRITE.csv WRITE.json OLD.json
                                rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE counter CSVs and the bench lines of those two
                                runs: the config2, config2_by_kernel and config4 entries of profiles/pmc_traffic.json
                                (OLD.json: the record to refresh; its other entries are kept), printed as JSON
"""
import collections
import csv
import glob
import json
import os
import re
import statistics
import sys


def bench_line(path):
    return json.loads([l for l in open(path) if l.startswith("{")][-1])


def short(name):
    m = re.search(r"(cn_strip_kernel<[^>]*>|stream_copy_kernel|soil_tables_kernel<[^>]*>|expand_code_bytes)", name)
    return m.group(1) if m else name[:60]


def bench(d):
    rows = [("ms_per_step", lambda b: b["ms_per_step"]),
            ("roofline.avg_launch_ms", lambda b: b["roofline"]["avg_launch_ms"]),
            ("also.avg_launch_ms", lambda b: b["also"]["avg_launch_ms"]),
            ("same-run plain copy, ms", lambda b: b["roofline"]["copy_ceiling"]["avg_ms"])]
    for side in ("parent", "new"):
        lines = [bench_line(p) for p in sorted(glob.glob(os.path.join(d, "bench_%s_[0-9].json" % side)))]
        print(side, len(lines), "runs; timed kernels", [b["roofline"]["kernel"] for b in lines],
              "self-check, differing pixels", [b.get("self_check", {}).get("differing") for b in lines])
        for name, get in rows:
            v = [get(b) for b in lines]
            print("  %-28s median %.4f (min %.4f - max %.4f, range %.4f)  %s" % (name, statistics.median(v), min(v), max(v),
                                                                                 max(v) - min(v), v))


def pairs(trace):
    rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
    names = [short(r["Kernel_Name"]) for r in rows]
    got = []
    for i in range(len(rows) - 1):
        if names[i].startswith("soil_tables_kernel") and names[i + 1].startswith("cn_strip_kernel<1,"):
            a, b = rows[i], rows[i + 1]
            got.append(((int(a["End_Timestamp"]) - int(a["Start_Timestamp"])) / 1e3,
                        (int(b["Start_Timestamp"]) - int(a["End_Timestamp"])) / 1e3,
                        (int(b["End_Timestamp"]) - int(b["Start_Timestamp"])) / 1e3, names[i + 1]))
    got = got[-20:]
    print("last %d prepare+strip pairs of the trace (%s), medians: prepare kernel %.2f us, gap to the strip kernel %.2f us, "
          "strip kernel %.2f us" % (len(got), got[-1][3], statistics.median(g[0] for g in got),
                                    statistics.median(g[1] for g in got), statistics.median(g[2] for g in got)))


def traffic(fetch_csv, fetch_json, write_csv, write_json, old):
    doc = json.load(open(old))
    new = {"config2_by_kernel": {}}
    for counter, f, line in (("FETCH_SIZE", fetch_csv, fetch_json), ("WRITE_SIZE", write_csv, write_json)):
        chosen = bench_line(line)["roofline"]["kernel"]
        per = collections.OrderedDict()
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] == counter:
                key = (int(r["Dispatch_Id"]), short(r["Kernel_Name"]))
                per[key] = per.get(key, 0.0) + float(r["Counter_Value"])
        order = sorted(per)
        names = [k[1] for k in order]
        first_copy = names.index("stream_copy_kernel") if "stream_copy_kernel" in names else len(order)
        strip = [per[k] for k in order[:first_copy] if k[1] == chosen][-4:]
        k18 = [per[k] for k in order if k[1].startswith("cn_strip_kernel<0, 3")]
        by_var = collections.defaultdict(list)
        for k in order:
            if k[1].startswith("cn_strip_kernel<1,"):
                by_var[k[1]].append(per[k])
        for kn, vals in by_var.items():
            t = new["config2_by_kernel"].setdefault(kn, {})
            t[counter + "_KiB"] = sum(vals) / len(vals)
            t[counter + "_dispatches"] = len(vals)
        for key, vals, kn in (("config2", strip, chosen),
                              ("config4", k18, next((n for n in names if n.startswith("cn_strip_kernel<0, 3")), ""))):
            if vals:
                t = new.setdefault(key, {"kernel": kn})
                t[counter + "_KiB"] = sum(vals) / len(vals)
                t[counter + "_dispatches"] = len(vals)
    correction = doc["copy"]["correction"]
    for key, t in list(new["config2_by_kernel"].items()) + [(k, new[k]) for k in ("config2", "config4") if k in new]:
        if "FETCH_SIZE_KiB" in t and "WRITE_SIZE_KiB" in t:
            t["hbm_bytes_per_launch"] = int((2 * t["FETCH_SIZE_KiB"] + t["WRITE_SIZE_KiB"]) * 1024)
            if key in ("config2", "config4"):
                t["correction"] = correction
    for key in ("config2_by_kernel", "config2", "config4"):
        if key in new and new[key]:
            doc[key] = new[key]
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    {"bench": bench, "pairs": pairs, "traffic": traffic}[sys.argv[1]](*sys.argv[2:])
