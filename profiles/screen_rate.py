"""Rate of read screening (moni_screen_run, both strands and strands = 1) on the benchmark's workload, beside moni_pml_run on the same reads in
the same process and from the same build (its kernel is the yardstick): the index bench.py caches, its 1 M x 150 bp reads, one context, 3 warm-up
steps and 10 timed steps.  Per leg: reads/s (wall time of the call), the HIP-event time of the whole run and of the walk kernel alone, their
minimum - maximum over the timed steps, and the time per LF step from the library's counters (screen_kernel walks 2 * strands strings per read,
pml_kernel one).  Prints one JSON line.

    python profiles/screen_rate.py [--cache DIR] [--base-len N --haps H] [--reads N] [--steps K] [--warmup W] [--window N --min-win N]

The index file must exist (a bench.py run with the same --base-len / --haps writes it); nothing is built here.
Counters: rocprofv3 --pmc <one counter> -- python profiles/screen_rate.py --steps 2 --warmup 1 --no-pml (a run of its own, no tracing beside it)."""
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
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--min-win", type=int, default=25)
    ap.add_argument("--no-pml", action="store_true", help="skip the moni_pml_run leg (profiling runs)")
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

    def calls(res):
        present = (res["flags"] & capi.SCREEN_PRESENT) != 0
        return {"present": int(present.sum()), "present_strand1": int((present & ((res["flags"] & capi.SCREEN_STRAND1) != 0)).sum()),
                "short": int(((res["flags"] & capi.SCREEN_SHORT) != 0).sum()), "mean_max_pml0": float(res["max_pml"][:, 0].mean()),
                "mean_d_max0": float(res["d_max"][:, 0].mean())}

    out = {"reads": a.reads, "read_len": a.read_len, "steps": a.steps, "warmup": a.warmup, "window": a.window, "min_win": a.min_win}
    out["screen"] = leg(lambda: ctx.screen_run(window=a.window, min_win=a.min_win))
    out["screen"].update(calls(ctx.screen_fetch()))
    out["screen_one_strand"] = leg(lambda: ctx.screen_run(window=a.window, min_win=a.min_win, strands=1))
    out["screen_one_strand"].update(calls(ctx.screen_fetch()))
    if not a.no_pml:
        out["pml"] = leg(lambda: ctx.pml_run(25))
        out["screen_over_pml_per_step"] = out["screen"]["ps_per_lf_step"] / out["pml"]["ps_per_lf_step"]
        out["screen_one_strand_over_pml_per_step"] = out["screen_one_strand"]["ps_per_lf_step"] / out["pml"]["ps_per_lf_step"]
        out["screen_over_pml_run"] = out["screen"]["run_ms_median"] / out["pml"]["run_ms_median"]
    print(json.dumps(out))
    ctx.close()
    idx.close()


if __name__ == "__main__":
    main()
