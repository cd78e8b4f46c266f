#!/usr/bin/env python3
"""Timeline of the pipelined ReSTIR DI bench from a rocprofv3 --kernel-trace CSV (streams overlap, so unlike frame_timeline.py it lists
every kernel of a window with its queue): the kernels of two steady-state frames with their offsets, and over 16 steady-state frames how
long the setup kernel ran beside a Part-1 traversal kernel and with no traversal kernel beside it (profiles/di_split/timeline.txt).
  usage: pipeline_timeline.py <kernel_trace.csv> <name of the frame's first kernel, e.g. k_di_part1_primary>"""
import csv
import sys

rows = [r for r in csv.DictReader(open(sys.argv[1])) if "<true>" not in r["Kernel_Name"]]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
for r in rows:
    r["s"], r["e"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    r["n"] = r["Kernel_Name"].split("(")[0].replace("void ", "")
first = [i for i, r in enumerate(rows) if sys.argv[2] in r["n"]]
a = first[len(first) // 2]
t0 = rows[a]["s"]
span = (rows[first[len(first) // 2 + 8]]["s"] - rows[first[len(first) // 2 - 8]]["s"]) / 16e3
print(f"frame period (mean of 16 steady-state frames): {span:.1f} us")
print(f"{'start':>10s} {'dur':>9s} {'end':>10s}  queue  kernel")
for r in rows:
    if t0 - 50_000 <= r["s"] <= t0 + 2 * span * 1e3:
        print(f"{(r['s'] - t0) / 1e3:10.1f} {(r['e'] - r['s']) / 1e3:9.1f} {(r['e'] - t0) / 1e3:10.1f}  {r.get('Queue_Id', '?'):>5s}  {r['n'][:48]}")


def covered(lo, hi, others):
    """length of [lo, hi) covered by the union of the intervals in `others`"""
    tot, cur = 0, lo
    for s, e in sorted(others):
        s, e = max(s, cur), min(e, hi)
        if e > s:
            tot += e - s
            cur = e
    return tot


lo_i, hi_i = first[len(first) // 2 - 8], first[len(first) // 2 + 8]
trav = [(r["s"], r["e"]) for r in rows if "k_di_part1" in r["n"] and "temporal" not in r["n"] or "k_di_part2_trace" in r["n"]]
alone, beside_primary, dur, n = 0.0, 0.0, 0.0, 0
prim = [(r["s"], r["e"]) for r in rows if "k_di_part1" in r["n"] and "temporal" not in r["n"]]
for r in rows[lo_i:hi_i]:
    if "k_di_part2_setup" in r["n"]:
        d = r["e"] - r["s"]
        alone += d - covered(r["s"], r["e"], trav); beside_primary += covered(r["s"], r["e"], prim); dur += d; n += 1
if n:
    print(f"setup kernel over {n} frames: {dur / n / 1e3:.1f} us, of which beside a Part-1 traversal kernel {beside_primary / n / 1e3:.1f} us, "
          f"with no traversal kernel (Part 1 / primary / trace) beside it {alone / n / 1e3:.1f} us")
for name in ("k_di_part1_primary", "k_di_part1_temporal", "k_di_part1<", "k_di_part2_setup", "k_di_part2_trace"):
    ds = [r["e"] - r["s"] for r in rows[lo_i:hi_i + 8] if name in r["n"]]
    if ds:
        print(f"{name:22s} mean {sum(ds) / len(ds) / 1e3:7.1f} us over {len(ds)} launches in the timed region")
