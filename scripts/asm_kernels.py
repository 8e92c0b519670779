#!/usr/bin/env python3
"""Compare the kernels of two `make asm` output directories, symbol by symbol.

    python scripts/asm_kernels.py OLD_DIR NEW_DIR [--rename OLD_SYMBOL=NEW_SYMBOL ...]

Every .s file of a directory is cut into per-kernel records keyed by the kernel's symbol:
the body (from `<symbol>:` to its `.Lfunc_end`), its `.amdhsa_kernel` .. `.end_amdhsa_kernel`
block and its entry in the `amdhsa.kernels` metadata. The per-file function index in local
labels (`.LBB<n>_<m>`, `.Lfunc_end<n>`) is dropped, and so are the comments (they name loop
headers by that index), so a kernel may move between files or change its place in one;
`.file`, `.ident` and `__hip_cuid` lie outside the records. A symbol
found in several files of a directory (a source compiled into two objects) must have one
record there. --rename compares OLD_SYMBOL's record with NEW_SYMBOL's, with the name
replaced wherever it appears (the kernel's own static LDS symbols included).

Prints one line per symbol -- identical / differs / only in OLD / only in NEW -- with the
files it was found in, then the totals. Exit status 1 if anything differs or is lost.
"""
import argparse
import glob
import os
import re
import sys

LABEL = re.compile(r"\.(LBB|Lfunc_end)\d+")
COMMENT = re.compile(r"[ \t]*;.*$", re.M)  # (they name blocks by the function index too)


def records(path):
    """{symbol: (body, descriptor, metadata)} of one .s file"""
    lines = open(path).read().split("\n")
    body, desc, meta = {}, {}, {}
    i, n = 0, len(lines)
    while i < n:
        m = re.match(r"\s+\.type\s+(\S+),@function", lines[i])
        if m and i + 1 < n and lines[i + 1].startswith(m.group(1) + ":"):
            sym, j = m.group(1), i + 1
            text, kd, in_kd = [], [], False
            while not re.match(r"\.Lfunc_end\d+:", lines[j]):
                s = lines[j]
                if re.match(r"\s+\.amdhsa_kernel\s", s):
                    in_kd = True
                (kd if in_kd else text).append(s)
                if re.match(r"\s+\.end_amdhsa_kernel", s):
                    in_kd = False
                j += 1
            if kd:  # (a plain device function has no descriptor: not a kernel)
                body[sym], desc[sym] = text, kd
            i = j
        elif lines[i].startswith("amdhsa.kernels:"):
            i += 1
            item = []
            while i < n and (lines[i].startswith("  ") or not lines[i].strip()):
                if lines[i].startswith("  - ") and item:
                    meta[_name(item)] = item
                    item = []
                item.append(lines[i])
                i += 1
            if item:
                meta[_name(item)] = item
            continue
        i += 1
    out = {}
    for sym in body:
        out[sym] = tuple(LABEL.sub(r".\1", COMMENT.sub("", "\n".join(part)))
                         for part in (body[sym], desc[sym], meta.get(sym, ["<no metadata>"])))
    return out


def _name(item):
    for s in item:
        m = re.match(r"\s+\.name:\s+(\S+)", s)
        if m:
            return m.group(1)
    return "?"


def scan(d):
    """{symbol: {record: [files]}} over the .s files of a directory"""
    out = {}
    for path in sorted(glob.glob(os.path.join(d, "*.s"))):
        for sym, rec in records(path).items():
            out.setdefault(sym, {}).setdefault(rec, []).append(os.path.basename(path))
    return out


def files(recs):
    return ",".join(f for fs in recs.values() for f in fs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    a = ap.parse_args()
    old, new = scan(a.old), scan(a.new)
    for pair in a.rename:
        o, nsym = pair.split("=")
        if o in old:  # (o[2:]: `_ZZ<name>E<var>` of a static LDS symbol holds the name without _Z)
            old[nsym] = {tuple(p.replace(o[2:], nsym[2:]) for p in rec): [f + " as " + o for f in fs]
                         for rec, fs in old.pop(o).items()}
    tot = {"identical": 0, "differs": 0, "only in OLD": 0, "only in NEW": 0}
    for sym in sorted(set(old) | set(new)):
        if sym not in new:
            verdict, where = "only in OLD", files(old[sym])
        elif sym not in old:
            verdict, where = "only in NEW", files(new[sym])
        else:
            same = len(old[sym]) == 1 and len(new[sym]) == 1 and set(old[sym]) == set(new[sym])
            verdict = "identical" if same else "differs"
            where = files(old[sym]) + " -> " + files(new[sym])
            if not same:
                parts = ("body", "descriptor", "metadata")
                ro, rn = next(iter(old[sym])), next(iter(new[sym]))
                where += " (" + ", ".join(p for p, x, y in zip(parts, ro, rn) if x != y) + ")"
        tot[verdict] += 1
        print(f"{verdict:12s} {sym}  [{where}]")
    print("total: " + ", ".join(f"{v} {k}" for k, v in tot.items()))
    return 1 if tot["differs"] or tot["only in OLD"] else 0


if __name__ == "__main__":
    sys.exit(main())
