#!/usr/bin/env python3
"""Parent against change from the raw lines of alternating tools/bench_grid_storms.py processes.

    python3 profiles/grid_fold/bench_compare.py profiles/grid_fold/bench_raw.jsonl

Each raw line is {"library": "parent" | "change", "run": n, "line": <the tool's JSON line>}.  A figure is the min_ms of
one leg at one (pattern, cell size) in one process.  For every figure: the five of each library, and where the median of
the change's five lies in the parent's own [min, max] -- the only margin there is for "unchanged"; a median below the
parent's minimum is reported as such and does not fail a figure.  The gate is the legs (m) and (w), the memset + sums +
finish trios of the plain and of the one-table calls; their sums kernels alone and the (s_k) legs are listed beside
them.
"""
import json
import statistics
import sys

GATE = ("m", "w")
BESIDE = ("m.kernel", "w.kernel", "s_1", "s_2", "s_4", "s_8")


def pick(t, leg):
    for key in leg.split("."):
        t = t[key]
    return float(t["min_ms"])


def main(path):
    rows = [json.loads(l) for l in open(path) if l.strip()]
    print("%-30s %-36s %-36s %8s  %s" % ("figure (min_ms)", "parent runs", "change runs", "N median", "verdict"))
    first = rows[0]["line"]["patterns"]
    outside = 0
    for legs, gate in ((GATE, True), (BESIDE, False)):
        print("# the gate" if gate else "# beside it (not part of the gate)")
        for leg in legs:
            for pattern in first:
                for grid in first[pattern]:
                    p = [pick(r["line"]["patterns"][pattern][grid], leg) for r in rows if r["library"] == "parent"]
                    n = [pick(r["line"]["patterns"][pattern][grid], leg) for r in rows if r["library"] == "change"]
                    mn = statistics.median(n)
                    verdict = "inside" if min(p) <= mn <= max(p) else "outside, faster" if mn < min(p) else "OUTSIDE, SLOWER"
                    outside += gate and verdict == "OUTSIDE, SLOWER"
                    print("%-30s %-36s %-36s %8.3f  %s" % ("%s %s %s" % (leg, pattern, grid.replace("grid_", "")),
                                                            " ".join("%g" % v for v in p), " ".join("%g" % v for v in n),
                                                            mn, verdict))
    same = all(t["words_and_bytes_equal_across_the_legs"] for r in rows for v in r["line"]["patterns"].values()
               for t in v.values())
    print("# words and bytes equal across the legs in all %d processes: %s" % (len(rows), same))
    print("# gate: %d of %d figures slower than the parent's range" % (outside,
                                                                       len(GATE) * sum(len(v) for v in first.values())))


if __name__ == "__main__":
    main(sys.argv[1])
