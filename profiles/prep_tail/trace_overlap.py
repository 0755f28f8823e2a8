#!/usr/bin/env python3
"""From a rocprofv3 kernel trace (csv): per-launch statistics of the named kernels, and for every slow launch of finish_prep_kernel what ran beside it."""
import collections
import csv
import statistics
import sys

path, out = sys.argv[1], sys.argv[2]
rows = []
for r in csv.DictReader(open(path)):
    n = r["Kernel_Name"].replace("void ", "")
    n = n[:n.index("(")] if "(" in n else n
    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), n, r.get("Queue_Id", "?"), r.get("Grid_Size", r.get("Grid_Size_X", "?"))))
rows.sort()
t_base = rows[0][0]
by = collections.defaultdict(list)
for s, e, n, q, g in rows:
    by[n].append((s, e, q, g))
with open(out, "w") as fh:
    for n in ("finish_prep_kernel", "finish_list_kernel", "finish_render_kernel", "plan_kernel", "select_kernel", "traceback_kernel", "align_kernel", "gather_lines_kernel"):
        v = by.get(n)
        if not v:
            continue
        by_grid = collections.defaultdict(list)
        for s, e, q, g in v:
            by_grid[g].append((e - s) / 1e6)
        for g, d in sorted(by_grid.items()):
            fh.write("%-24s grid %-10s launches %3d  min %.3f  median %.3f  max %.3f  mean %.3f ms\n" % (n, g, len(d), min(d), statistics.median(d), max(d), sum(d) / len(d)))
    prep = by.get("finish_prep_kernel", [])
    if prep:
        med = statistics.median([(e - s) for s, e, _, _ in prep])
        fh.write("\nlaunches of finish_prep_kernel in order (ms since the first kernel; duration; queue), and for the slow ones the kernels that overlap them:\n")
        for i, (s, e, q, g) in enumerate(prep):
            fh.write("  #%d at %.3f  %.3f ms  queue %s grid %s\n" % (i, (s - t_base) / 1e6, (e - s) / 1e6, q, g))
            if e - s > 2 * med:
                for s2, e2, n2, q2, g2 in rows:
                    if e2 > s and s2 < e and not (s2 == s and n2 == "finish_prep_kernel"):
                        fh.write("        beside it: %-60s queue %s  from %+.3f to %+.3f ms (relative to its start), %.3f ms long\n" % (n2[:60], q2, (s2 - s) / 1e6, (e2 - s) / 1e6, (e2 - s2) / 1e6))
print(open(out).read())
