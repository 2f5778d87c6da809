"""Idle time between consecutive dispatches in a rocprofv3
kernel_trace.csv: for each pair of kernels that follow each other (by
start stamp), the gap from the end of the first to the start of the
second, grouped by the two kernel names.

Usage: python tools/kgaps.py <kernel_trace.csv> [skip]
skip: leading dispatches left out (set-up and warm-up; default 0)
"""
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
skip = int(sys.argv[2]) if len(sys.argv) > 2 else 0
ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]),
             r["Kernel_Name"]) for r in rows)[skip:]


def short(name):
    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    return name.split("(")[0][:40]


pairs = {}
for (s0, e0, n0), (s1, e1, n1) in zip(ev, ev[1:]):
    pairs.setdefault((short(n0), short(n1)), []).append(s1 - e0)
busy = sum(e - s for s, e, _ in ev)
span = ev[-1][1] - ev[0][0]
print("%d dispatches: span %.2f ms, busy %.2f ms, idle %.2f ms (%.1f%%)"
      % (len(ev), span / 1e6, busy / 1e6, (span - busy) / 1e6,
         100.0 * (span - busy) / span))
print("%-40s -> %-40s %7s %9s %9s %9s" % ("kernel", "next kernel", "pairs",
                                          "mean us", "median us", "p95 us"))
for (a, b), g in sorted(pairs.items(), key=lambda kv: -len(kv[1])):
    g.sort()
    print("%-40s -> %-40s %7d %9.2f %9.2f %9.2f"
          % (a, b, len(g), sum(g) / len(g) / 1e3, g[len(g) // 2] / 1e3,
             g[int(len(g) * 0.95)] / 1e3))
