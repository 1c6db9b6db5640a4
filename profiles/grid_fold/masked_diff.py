#!/usr/bin/env python3
"""What is left of a kernel's difference between two builds when register numbers do not count.

    python3 profiles/grid_fold/masked_diff.py PARENT_DIR CHANGE_DIR

The directories and the kernel texts are those of profiles/core_split/same_kernels.py.  For every kernel that both
builds hold and whose text differs: every s<n>, v<n>, s[a:b] and v[a:b] becomes R, and the lines that still differ are
printed (a line moved shows as one - and one +).
"""
import difflib
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "core_split"))
import same_kernels  # noqa: E402

REG = re.compile(r"\b[sv]\[\d+:\d+\]|\b[sv]\d+\b|\$[sv]gpr\d+(_[sv]gpr\d+)*")


def main(parent_dir, change_dir):
    a, b = same_kernels.kernels(parent_dir), same_kernels.kernels(change_dir)
    for sym in sorted(set(a) & set(b)):
        if a[sym][1:] == b[sym][1:]:
            continue
        ta = [REG.sub("R", l) for l in a[sym][1] + a[sym][2]]
        tb = [REG.sub("R", l) for l in b[sym][1] + b[sym][2]]
        d = [l for l in difflib.unified_diff(ta, tb, lineterm="", n=0) if not l.startswith(("---", "+++", "@@"))]
        print("%s: %d and %d lines, %d differ with registers masked" % (sym, len(ta), len(tb), len(d)))
        for l in d:
            print("    " + l)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
