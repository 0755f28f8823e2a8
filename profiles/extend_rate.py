"""Rate of extend mode (moni_extend_run) on the benchmark's workload, beside moni_align_run on the same reads from the same build (for
scale only): the index bench.py caches, its 1 M x 150 bp reads, one context, 3 warm-up steps and 10 timed steps, wall time and the
HIP-event kernel time of the steps.  Prints one JSON line.

    python profiles/extend_rate.py [--cache DIR] [--base-len N --haps H] [--reads N] [--steps K] [--warmup W]

The index file must exist (a bench.py run with the same --base-len / --haps writes it); nothing is built here.
Per-kernel split: rocprofv3 --kernel-trace --stats -- python profiles/extend_rate.py --steps 2 --warmup 1 --no-align"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache", default="/tmp/moni_bench_cache")
    ap.add_argument("--base-len", type=int, default=61420004)
    ap.add_argument("--haps", type=int, default=12)
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-align", action="store_true", help="skip the moni_align_run leg (profiling runs)")
    a = ap.parse_args()
    from moni_align_amd import capi, synth
    path = os.path.join(a.cache, "idx_%d_%d_lifted_0.mfi" % (a.base_len, a.haps))
    if not os.path.exists(path):
        sys.exit("no cached index %s: run bench.py with the same --base-len / --haps first" % path)
    pg = synth.make_pangenome(a.base_len, a.haps, seed=19, var_seed=12)
    reads = synth.make_reads(pg, a.reads, a.read_len, seed=150)
    del pg
    names, noff = synth.make_names(a.reads)
    offs = np.arange(0, (a.reads + 1) * a.read_len, a.read_len, dtype=np.uint64)
    quals = np.full(reads.size, ord("I"), dtype=np.uint8)
    idx = capi.Index(path=path, device=0)
    ctx = capi.Ctx(idx)
    ctx.upload(reads.reshape(-1), offs)

    def leg(fn, key):
        for _ in range(a.warmup):
            fn()
        wall, kern, last = [], [], None
        for _ in range(a.steps):
            t0 = time.perf_counter()
            n, st = fn()
            wall.append(time.perf_counter() - t0)
            kern.append(st[key])
            last = (n, st)
        w = float(np.median(wall))
        return {"reads_per_s": a.reads / w, "wall_s_median": w, "wall_s_min": min(wall), "wall_s_max": max(wall), "kernel_s_median": float(np.median(kern)),
                "text_bytes": last[0]}, last[1]

    ext, st = leg(lambda: ctx.extend_run(names, noff, quals, want_text=False), "t_kernel")
    out = {"reads": a.reads, "read_len": a.read_len, "steps": a.steps, "warmup": a.warmup, "extend": ext,
           "extended": st["extended"], "records": st["records"], "dp_tasks": st["dp_tasks"], "dp_cells": st["dp_cells"]}
    if not a.no_align:
        out["align"], _ = leg(lambda: ctx.align_run(names, noff, quals, want_text=False), "t_dp_kernel")
    print(json.dumps(out))
    ctx.close()
    idx.close()


if __name__ == "__main__":
    main()
