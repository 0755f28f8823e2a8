"""Rate of pseudo-matching lengths (moni_pml_run) on the benchmark's workload, beside moni_ms_run on the same reads in the same process and
from the same build (its kernel is the yardstick): the index bench.py caches, its 1 M x 150 bp reads, one context, 3 warm-up steps and
10 timed steps.  Per leg: reads/s (wall time of the call), the HIP-event time of the whole run and of the walk kernel alone, their
minimum - maximum over the timed steps, and the time per LF step from the library's counters (pml_kernel walks one strand, ms_lf_kernel
two).  Prints one JSON line.

    python profiles/pml_rate.py [--cache DIR] [--base-len N --haps H] [--reads N] [--steps K] [--warmup W] [--thr T]

The index file must exist (a bench.py run with the same --base-len / --haps writes it); nothing is built here.
Per-kernel split: rocprofv3 --kernel-trace --stats -- python profiles/pml_rate.py --steps 2 --warmup 1 --no-ms"""
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
    ap.add_argument("--thr", type=int, default=25)
    ap.add_argument("--no-ms", action="store_true", help="skip the moni_ms_run leg (profiling runs)")
    a = ap.parse_args()
    from moni_align_amd import capi, synth
    path = os.path.join(a.cache, "idx_%d_%d_lifted_0.mfi" % (a.base_len, a.haps))
    if not os.path.exists(path):
        sys.exit("no cached index %s: run bench.py with the same --base-len / --haps first" % path)
    pg = synth.make_pangenome(a.base_len, a.haps, seed=19, var_seed=12)
    reads = synth.make_reads(pg, a.reads, a.read_len, seed=150)
    del pg
    offs = np.arange(0, (a.reads + 1) * a.read_len, a.read_len, dtype=np.uint64)
    idx = capi.Index(path=path, device=0)
    ctx = capi.Ctx(idx)
    ctx.upload(reads.reshape(-1), offs)

    def leg(fn):
        for _ in range(a.warmup):
            fn()
        wall, run_ms, walk_ms = [], [], []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            fn()
            wall.append(time.perf_counter() - t0)
            run_ms.append(ctx.kernel_ms(6))
            walk_ms.append(ctx.kernel_ms(0))
        c = ctx.counters()
        steps, jumps = int(c[0]), int(c[1])
        w, k = float(np.median(wall)), float(np.median(walk_ms))
        return {"reads_per_s": a.reads / w, "wall_ms_median": w * 1e3, "wall_ms_min": min(wall) * 1e3, "wall_ms_max": max(wall) * 1e3,
                "run_ms_median": float(np.median(run_ms)), "run_ms_min": min(run_ms), "run_ms_max": max(run_ms),
                "walk_kernel_ms_median": k, "walk_kernel_ms_min": min(walk_ms), "walk_kernel_ms_max": max(walk_ms),
                "lf_steps": steps, "jumps": jumps, "ps_per_lf_step": k * 1e9 / steps, "ps_per_lf_step_min": min(walk_ms) * 1e9 / steps,
                "ps_per_lf_step_max": max(walk_ms) * 1e9 / steps}

    out = {"reads": a.reads, "read_len": a.read_len, "steps": a.steps, "warmup": a.warmup, "thr": a.thr, "pml": leg(lambda: ctx.pml_run(a.thr))}
    _, mx, hits = ctx.pml_fetch(want_lengths=False)
    out["reads_with_a_hit"] = int((hits > 0).sum())
    out["mean_read_max"] = float(mx.mean())
    if not a.no_ms:
        out["ms"] = leg(ctx.ms_run)
        out["pml_over_ms_per_step"] = out["pml"]["ps_per_lf_step"] / out["ms"]["ps_per_lf_step"]
        out["pml_over_ms_run"] = out["pml"]["run_ms_median"] / out["ms"]["run_ms_median"]
    print(json.dumps(out))
    ctx.close()
    idx.close()


if __name__ == "__main__":
    main()
