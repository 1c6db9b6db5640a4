#!/usr/bin/env python3
"""Parent against change from the raw lines of alternating bench.py processes.

    python3 profiles/core_split/bench_compare.py profiles/core_split/bench_raw.jsonl

Each raw line is {"library": "parent" | "change", "run": n, "line": <bench.py's JSON line>}.  For every figure: the
runs of each library, the medians, and where the change's median lies in the parent's own [min, max] -- the only
margin there is.  For `value` (Gpx/s) higher is better, for the times lower.
"""
import json
import statistics
import sys

FIGURES = (("value", True), ("ms_per_step", False), ("roofline.median_launch_ms", False),
           ("also.median_launch_ms", False))


def pick(line, path):
    for key in path.split("."):
        line = line[key]
    return float(line)


def main(path):
    rows = [json.loads(l) for l in open(path) if l.strip()]
    print("%-28s %-44s %-44s %9s %9s  %s" % ("figure", "parent runs", "change runs", "P median", "N median", "verdict"))
    for fig, higher in FIGURES:
        p = [pick(r["line"], fig) for r in rows if r["library"] == "parent"]
        n = [pick(r["line"], fig) for r in rows if r["library"] == "change"]
        mp, mn = statistics.median(p), statistics.median(n)
        if min(p) <= mn <= max(p):
            verdict = "inside"
        else:
            better = (mn > max(p)) == higher
            verdict = "outside, better" if better else "OUTSIDE, WORSE"
        print("%-28s %-44s %-44s %9.4f %9.4f  %s" % (fig, " ".join("%g" % v for v in p), " ".join("%g" % v for v in n),
                                                      mp, mn, verdict))
    kernels = sorted({(r["library"], r["line"]["roofline"]["kernel"], r["line"]["also"]["kernel"]) for r in rows})
    for lib, k2, k18 in kernels:
        print("# %s: config 2 ran %s, config 4 ran %s" % (lib, k2, k18))


if __name__ == "__main__":
    main(sys.argv[1])
