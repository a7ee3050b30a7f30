#!/usr/bin/env python3
"""Per-kernel comparison of two builds' device assembly (the -save-temps=obj .s files csrc/Makefile keeps).

  tools/kernel_isa_diff.py <build dir | file.s> <build dir | file.s> [--only-different]

A directory stands for every *-hip-amdgcn-amd-amdhsa-*.s in it; kernels are matched by symbol across all files of a side,
so a kernel that moved to another translation unit still finds its partner.  Per symbol: identical / DIFFERENT / only in
A / only in B, the instruction counts and the .amdhsa_ register, LDS and scratch figures of both sides.  A body is the text
from `<symbol>:` to `.Lfunc_end`, comments stripped and `.LBB<n>_` rewritten to `.LBB_`; it is compared as text, nothing is
looked for.  Exit status 1 if anything differs or is on one side only.
"""
import glob
import os
import re
import sys

FIGURES = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(text):
    """{symbol: (normalised body lines, {figure: value})} of one .s file's text."""
    lines, figures, sym = text.splitlines(), {}, None
    for line in lines:
        tok = line.split()
        if len(tok) >= 2 and tok[0] == ".amdhsa_kernel":
            sym = tok[1]
            figures[sym] = {}
        elif tok and tok[0] == ".end_amdhsa_kernel":
            sym = None
        elif sym and len(tok) >= 2 and tok[0][len(".amdhsa_"):] in FIGURES:
            figures[sym][tok[0][len(".amdhsa_"):]] = tok[1]
    found = {}
    for sym in figures:
        start = next((i for i, line in enumerate(lines) if line.startswith(sym + ":")), None)
        if start is None:
            continue
        end = next((i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end")), len(lines))
        body = (re.sub(r"\.LBB\d+_", ".LBB_", line.split(";", 1)[0].strip()) for line in lines[start + 1:end])
        found[sym] = ([line for line in body if line], figures[sym])
    return found


def load(path):
    files = sorted(glob.glob(os.path.join(path, "*-hip-amdgcn-amd-amdhsa-*.s"))) if os.path.isdir(path) else [path]
    found = {}
    for f in files:
        with open(f) as fh:
            for sym, k in kernels(fh.read()).items():
                # a header's internal-linkage kernel is emitted by every file that uses it: one entry while the copies agree
                if sym in found and found[sym] != k:
                    sym += "@" + os.path.basename(f).split("-hip-")[0]
                found[sym] = k
    return found


def compare(a, b):
    """[(symbol, verdict, instructions_a, instructions_b, figures_a, figures_b)] by symbol; a missing side has None."""
    def n(side, sym):
        return sum(1 for x in side[sym][0] if not x.endswith(":") and not x.startswith(".")) if sym in side else None
    rows = []
    for sym in sorted(set(a) | set(b)):
        if sym in a and sym in b:
            verdict = "identical" if a[sym][0] == b[sym][0] else "DIFFERENT"
        else:
            verdict = "only in A" if sym in a else "only in B"
        rows.append((sym, verdict, n(a, sym), n(b, sym), a[sym][1] if sym in a else {}, b[sym][1] if sym in b else {}))
    return rows


def main(argv):
    args = [x for x in argv if not x.startswith("--")]
    if len(args) != 2:
        sys.exit(__doc__)
    rows = compare(load(args[0]), load(args[1]))
    bad = 0
    for sym, verdict, na, nb, fa, fb in rows:
        changed = verdict != "identical" or fa != fb
        bad += changed
        if changed or "--only-different" not in argv:
            figs = " ".join("%s=%s|%s" % (k.split("_fixed")[0].replace("next_free_", ""), fa.get(k, "-"), fb.get(k, "-")) for k in FIGURES)
            print("%-10s %s insns=%s|%s %s%s" % (verdict, sym, na, nb, figs, "  FIGURES CHANGED" if fa and fb and fa != fb else ""))
    print("%d kernels, %d not identical or on one side only" % (len(rows), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
