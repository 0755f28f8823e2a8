"""Rate of the exact-match queries (moni_locate_run) on the benchmark's workload, beside moni_ms_run on the same batches in the same process and
from the same build (its kernel is the yardstick): the index bench.py caches, its 1 M x 150 bp reads and 1 M 32-base pieces cut from them, both
resident, one context, 3 warm-up steps and 10 timed steps.  Legs: count only, one strand, on the whole reads (most die early: the price of the
early exit); the same on the pieces (most occur); max_occ = 16 on the pieces; moni_ms_run on either batch.  Per leg: wall time of the call, the
HIP-event time of the whole run, of count_kernel / ms_lf_kernel and of locate_walk_kernel, their minimum - maximum over the timed steps, and from
the library's counters the search steps, the fast rows fetched per step, the steps on the general path, the phi steps and the time per step.
Prints one JSON line.

    python profiles/locate_rate.py [--cache DIR] [--base-len N --haps H] [--reads N] [--steps K] [--warmup W] [--piece L] [--max-occ M]

The index file must exist (a bench.py run with the same --base-len / --haps writes it); nothing is built here."""
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
    ap.add_argument("--piece", type=int, default=32)
    ap.add_argument("--max-occ", type=int, default=16)
    a = ap.parse_args()
    from moni_align_amd import capi, synth
    path = os.path.join(a.cache, "idx_%d_%d_lifted_0.mfi" % (a.base_len, a.haps))
    if not os.path.exists(path):
        sys.exit("no cached index %s: run bench.py with the same --base-len / --haps first" % path)
    pg = synth.make_pangenome(a.base_len, a.haps, seed=19, var_seed=12)
    reads = synth.make_reads(pg, a.reads, a.read_len, seed=150)
    del pg
    at = np.random.default_rng(32).integers(0, a.read_len - a.piece + 1, size=a.reads)
    pieces = reads[np.arange(a.reads)[:, None], at[:, None] + np.arange(a.piece)[None, :]]
    idx = capi.Index(path=path, device=0)
    ctx = capi.Ctx(idx)
    ctx.upload(reads.reshape(-1), np.arange(0, (a.reads + 1) * a.read_len, a.read_len, dtype=np.uint64))
    ctx.swap(0)                                  # the reads parked in slot 0, the pieces resident
    ctx.upload(np.ascontiguousarray(pieces).reshape(-1), np.arange(0, (a.reads + 1) * a.piece, a.piece, dtype=np.uint64))

    def leg(fn, walk=True):
        for _ in range(a.warmup):
            fn()
        wall, run_ms, main_ms, walk_ms = [], [], [], []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            fn()
            wall.append(time.perf_counter() - t0)
            run_ms.append(ctx.kernel_ms(6))
            main_ms.append(ctx.kernel_ms(0))
            if walk:
                walk_ms.append(ctx.kernel_ms(3))
        c = [int(x) for x in ctx.counters()]
        mm = lambda v, k: {k + "_median": float(np.median(v)), k + "_min": float(min(v)), k + "_max": float(max(v))}
        out = {"steps": c[0]}
        out.update(mm([w * 1e3 for w in wall], "wall_ms"))
        out.update(mm(run_ms, "run_ms"))
        out.update(mm(main_ms, "main_kernel_ms"))
        out.update(mm([k * 1e9 / c[0] for k in main_ms], "ps_per_step"))
        if walk:
            out.update(mm(walk_ms, "walk_kernel_ms"))
            out.update({"rows": c[1], "rows_per_step": c[1] / c[0], "general_steps": c[3], "phi_steps": c[2]})
        else:
            out["jumps"] = c[1]
        return out

    def found():
        res = ctx.locate_fetch(want_occ=False)[0]
        return {"patterns_that_occur": int((res["count"] > 0).sum()), "mean_matched": float(res["matched"].mean()), "positions": int(res["n_occ"].sum()),
                "max_count": int(res["count"].max())}

    out = {"reads": a.reads, "read_len": a.read_len, "piece": a.piece, "max_occ": a.max_occ, "steps": a.steps, "warmup": a.warmup}
    out["pieces_count"] = leg(lambda: ctx.locate_run(1, 0))
    out["pieces_count"].update(found())
    out["pieces_locate"] = leg(lambda: ctx.locate_run(1, a.max_occ))
    out["pieces_locate"].update(found())
    out["pieces_ms"] = leg(ctx.ms_run, walk=False)
    ctx.swap(0)                                  # the whole reads resident
    out["reads_count"] = leg(lambda: ctx.locate_run(1, 0))
    out["reads_count"].update(found())
    out["reads_ms"] = leg(ctx.ms_run, walk=False)
    for k in ("pieces", "reads"):
        out[k + "_count_over_ms_per_step"] = out[k + "_count"]["ps_per_step_median"] / out[k + "_ms"]["ps_per_step_median"]
    print(json.dumps(out))
    ctx.close()
    idx.close()


if __name__ == "__main__":
    main()
