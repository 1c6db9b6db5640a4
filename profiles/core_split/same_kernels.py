#!/usr/bin/env python3
"""Compares the device assembly of two builds kernel by kernel, whatever file a kernel was compiled from.

    for f in gcn10_amd/csrc/*.hip; do
        hipcc <the Makefile's HIPFLAGS> -Igcn10_amd/csrc --cuda-device-only -S -o DIR/$(basename $f .hip).s $f
    done                                        # once in a checkout of the parent (PARENT_DIR), once here (CHANGE_DIR)
    python3 profiles/core_split/same_kernels.py PARENT_DIR CHANGE_DIR > profiles/core_split/same_kernels.txt

A kernel is a symbol with an .amdhsa_kernel block.  Its text is everything from its label to its .Lfunc_end label, and
its .amdhsa_kernel block; the function-index part of local labels (.LBB<n>_, .Lfunc_end<n>, ...) is normalised, since
it counts the functions in front of the kernel in its file.  One line per kernel: verdict, parent file, new file,
demangled name.  A kernel whose text differs is followed by a unified diff; a kernel in one build only is listed as
such.  Exit status 1 unless both builds hold the same kernels with the same text.
"""
import difflib
import glob
import os
import re
import subprocess
import sys

LOCAL = re.compile(r"\.L([A-Za-z_]+?)\d+(_\d+)?\b")


COMMENT = re.compile(r"\bBB\d+_")       # "; in Loop: Header=BB<n>_3": the same index in the compiler's comments


def normal(line):
    line = COMMENT.sub("BB_", LOCAL.sub(lambda m: ".L%s%s" % (m.group(1), m.group(2) or ""), line.rstrip()))
    return re.sub(r"\s+", " ", line)        # (a comment's column moves with the length of the label in front of it)


def kernels(directory):
    """{symbol: (file, [text lines], [amdhsa lines])}"""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        lines = open(path, errors="replace").read().split("\n")
        names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
        for name in names:
            start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
            end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
            h0 = next(i for i, l in enumerate(lines) if l.strip() == ".amdhsa_kernel " + name)
            h1 = next(i for i in range(h0, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
            out[name] = (os.path.basename(path), [normal(l) for l in lines[start:end + 1]],
                         [normal(l) for l in lines[h0:h1 + 1]])
    return out


def main(parent_dir, change_dir):
    a, b = kernels(parent_dir), kernels(change_dir)
    syms = sorted(set(a) | set(b))
    nice = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")
    same = differ = 0
    for sym, name in zip(syms, nice):
        name = re.sub(r"\(.*\)$", "", name.replace("(anonymous namespace)::", ""))
        if sym not in a or sym not in b:
            differ += 1
            print("ONLY-IN-%s %-26s %s" % ("PARENT" if sym in a else "CHANGE", (a.get(sym) or b.get(sym))[0], name))
            continue
        (fa, ta, ha), (fb, tb, hb) = a[sym], b[sym]
        if ta == tb and ha == hb:
            same += 1
            print("same     %-26s %-26s %5d lines  %s" % (fa, fb, len(ta), name))
            continue
        differ += 1
        print("DIFFERS  %-26s %-26s %s" % (fa, fb, name))
        for line in difflib.unified_diff(ta + ha, tb + hb, fa, fb, lineterm="", n=2):
            print("    " + line)
    print("%d kernels in the parent, %d in the change: %d same, %d differ or are missing" % (len(a), len(b), same, differ))
    return 0 if differ == 0 and len(a) == len(b) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
