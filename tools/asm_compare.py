#!/usr/bin/env python3
"""Compares two device assembly listings of fyprt.hip kernel by kernel; runs without a GPU.

Each listing is what csrc/build.sh's hipcc line gives with `--cuda-device-only -S -o NAME.s` in place of `-c -o fyprt.o`.  A listing is
split into its kernels; of a kernel's text only labels and instructions are kept, comments and directives dropped, and basic-block labels
renumbered in order of first appearance (their numbers carry the function's ordinal, which moves when kernels are added or removed).
Kernels are paired by mangled name; a kernel whose name changed is paired through --map, a file of `old<TAB>new` lines of demangled
names without return type and parameter list, as this tool prints them.  For every pair: identical or not, the instruction counts, and
for pairs that differ the resource figures of both sides (VGPRs, SGPRs, scratch, LDS, occupancy).

  usage: asm_compare.py OLD.s NEW.s [--map FILE] [--only SUBSTRING] [--diff]
Prints one line per pair that --only selects (default: pairs that differ or were renamed) and a summary; exit status 1 if any pair differs
or a kernel has no partner."""
import argparse
import difflib
import re
import subprocess
import sys

RESOURCES = (("VGPR", "NumVgprs"), ("SGPR", "TotalNumSgprs"), ("scratch", "ScratchSize"), ("LDS", "LDSByteSize"), ("waves", "Occupancy"))


def kernels_of(path):
    """{mangled name: (normalised lines, instruction count, {resource: value})} of the kernels (not the device functions) in a listing."""
    funcs, info, kernel_names = {}, {}, set()
    name, body, last = None, None, None
    for raw in open(path, errors="replace"):
        line = raw.rstrip("\n")
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            name, body = m.group(1), []
            continue
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            kernel_names.add(m.group(1))
        if name is not None:
            if line.startswith(".Lfunc_end"):
                funcs[name], last, name = body, name, None
                continue
            code = line.split(";", 1)[0].rstrip()
            if not code.strip() or code.lstrip().startswith(".") and not code.rstrip().endswith(":"):
                continue                                              # blank, comment or directive (a label line ends in a colon)
            if code.strip() == name + ":":
                continue
            body.append(code.strip())
            continue
        m = re.match(r";\s*(\w+):\s*(\d+)", line)
        if m and last is not None:
            info.setdefault(last, {}).setdefault(m.group(1), int(m.group(2)))
    out = {}
    for n in kernel_names:
        labels = {}
        lines = [re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), l) for l in funcs.get(n, [])]
        out[n] = (lines, sum(not l.endswith(":") for l in lines), info.get(n, {}))
    return out


def demangle(names):
    names = list(names)
    text = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {n: re.sub(r"\(.*", "", d).replace("void ", "") for n, d in zip(names, text)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old"); ap.add_argument("new")
    ap.add_argument("--map"); ap.add_argument("--only"); ap.add_argument("--diff", action="store_true")
    a = ap.parse_args()
    old, new = kernels_of(a.old), kernels_of(a.new)
    dold, dnew = demangle(old), demangle(new)
    pairs = [(n, n) for n in old if n in new]
    if a.map:
        by_old, by_new = {d: n for n, d in dold.items()}, {d: n for n, d in dnew.items()}
        for line in open(a.map):
            if line.strip() and not line.startswith("#"):
                o, n = (s.strip() for s in line.rstrip("\n").split("\t"))
                if o not in by_old or n not in by_new:
                    sys.exit(f"--map names a kernel that is not in the listings: {line.strip()}")
                pairs.append((by_old[o], by_new[n]))
    lone = sorted({dold[n] for n in old} - {dold[o] for o, _ in pairs}) + sorted({dnew[n] for n in new} - {dnew[n] for _, n in pairs})
    same = differ = 0
    for o, n in sorted(pairs, key=lambda p: dnew[p[1]]):
        (lo, io, ro), (ln, in_, rn) = old[o], new[n]
        ident = lo == ln
        same += ident; differ += not ident
        shown = a.only in dold[o] or a.only in dnew[n] if a.only else (not ident or o != n)
        if not shown:
            continue
        names = dold[o] if o == n else f"{dold[o]}  ->  {dnew[n]}"
        res = "" if ident else "  " + "  ".join(f"{k} {ro.get(f, '?')}/{rn.get(f, '?')}" for k, f in RESOURCES)
        print(f"{names}: instructions {io}/{in_}, identical {'yes' if ident else 'no'}{res}")
        if a.diff and not ident:
            sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(lo, ln, "old", "new", lineterm="", n=1))
    for d in lone:
        print(f"without a partner: {d}")
    print(f"{len(pairs)} kernel pairs: {same} identical, {differ} differ; {len(lone)} without a partner")
    return 1 if differ or lone else 0


if __name__ == "__main__":
    sys.exit(main())
