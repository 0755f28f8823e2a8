#!/usr/bin/env python3
"""The tail criterion: no launch of finish_prep_kernel in the change's trace may exceed twice the median launch of the parent's trace at the same grid (sub-batch) size."""
import re
import sys


def rows(path):
    out = {}
    for line in open(path):
        m = re.match(r"finish_prep_kernel\s+grid (\S+)\s+launches\s+(\d+)\s+min ([\d.]+)\s+median ([\d.]+)\s+max ([\d.]+)", line)
        if m:
            out[m.group(1)] = (int(m.group(2)), float(m.group(3)), float(m.group(4)), float(m.group(5)))
    return out


parent, change = rows(sys.argv[1]), rows(sys.argv[2])
ok = bool(change)
for g, (n, mn, med, mx) in sorted(change.items()):
    p = parent.get(g)
    if not p:
        print("grid %s: %d launches of the change (min %.3f median %.3f max %.3f ms), none of the parent" % (g, n, mn, med, mx))
        ok = False
        continue
    good = mx <= 2 * p[2]
    ok = ok and good
    print("grid %s: parent %d launches min %.3f median %.3f max %.3f ms | change %d launches min %.3f median %.3f max %.3f ms | bound 2 x %.3f = %.3f ms: %s" %
          (g, p[0], p[1], p[2], p[3], n, mn, med, mx, p[2], 2 * p[2], "met" if good else "MISSED"))
sys.exit(0 if ok else 1)
