#!/usr/bin/env python3
"""Kernel resource table from hipcc's -Rpass-analysis=kernel-resource-usage remarks (stderr of the build).

    hipcc <the Makefile's HIPFLAGS> -Igcn10_amd/csrc -Rpass-analysis=kernel-resource-usage -c FILE.hip 2> FILE.remarks
    python3 profiles/core_split/resource_table.py *.remarks > table.txt

One line per kernel symbol (demangled), sorted by file and name: source file, SGPRs, VGPRs, AGPRs, scratch bytes per lane, SGPR and VGPR
spills, LDS bytes per block, occupancy in waves per SIMD.  Only the files named in FILES are listed.
"""
import re
import subprocess
import sys

FILES = ("gcn10_strip.hip", "gcn10_soil_tile.hip", "gcn10_reference_fns.hip", "gcn10_deflate.hip",
         "gcn10_deflate_fused.hip", "gcn10_inflate.hip", "gcn10_lzw.hip")
KEYS = (("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"),
        ("SGPRs Spill", "sspill"), ("VGPRs Spill", "vspill"), ("LDS Size [bytes/block]", "lds"),
        ("Occupancy [waves/SIMD]", "occ"))


def main(paths):
    rows, cur = {}, None
    pat = re.compile(r"([^/\s:]+\.hip):\d+:\d+: remark:\s+(.+?): (\S+) \[-Rpass-analysis")
    for path in paths:
        for line in open(path, errors="replace"):
            m = pat.search(line)
            if not m or m.group(1) not in FILES:
                continue
            src, key, val = m.groups()
            if key == "Function Name":
                cur = rows.setdefault((src, val), {})
            elif cur is not None:
                cur[key] = val
    names = subprocess.run(["c++filt"], input="\n".join(sym for _, sym in rows), capture_output=True,
                           text=True).stdout.split("\n")
    out = []
    for ((src, _), vals), name in zip(rows.items(), names):
        name = name.replace("(anonymous namespace)::", "")
        name = re.sub(r"\(.*\)$", "", name)         # the parameter list names the parameter struct only
        out.append((src, name, "%-24s %s  %s" % (src, " ".join("%s=%s" % (short, vals.get(key, "?")) for key, short in KEYS),
                                                   name)))
    print("\n".join(line for _, _, line in sorted(out)))


if __name__ == "__main__":
    main(sys.argv[1:])
