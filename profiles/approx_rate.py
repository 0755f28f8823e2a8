"""Rate of the k-mismatch queries (moni_approx_run) on the benchmark's workload, beside count_kernel (moni_locate_run, count only) on the same
batches in the same process and from the same build - its time per search step is the yardstick: the index bench.py caches, 1 M 32-base pieces of
its reads at k = 1 and 2, and the 1 M x 150 bp reads at k = 1, both resident, one context, 3 warm-up steps and 10 timed steps per leg.  Every
workload runs with chunk_len 8, 16, 32 and 1 << 30 (one lane per task: the baseline of the cut).  Per leg: wall time of the call, the HIP-event
time of the whole run, of the exact pass and of the tree pass (minimum, median and maximum over the timed steps), and from the library's counters
the steps of the search tree, the time per tree step, the fast rows fetched per step and the share of tasks with complete = 0.  Counts only
(max_hits 0): the search is what is measured.  Prints one JSON line.

    python profiles/approx_rate.py [--cache DIR] [--base-len N --haps H] [--reads N] [--steps K] [--warmup W] [--piece L] [--max-steps N]

The index file must exist (a bench.py run with the same --base-len / --haps writes it); nothing is built here."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNKS = (8, 16, 32, 1 << 30)


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
    ap.add_argument("--max-steps", type=int, default=None, help="per piece (default: the library's)")
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
    mm = lambda v, k: {k + "_median": float(np.median(v)), k + "_min": float(min(v)), k + "_max": float(max(v))}

    def leg(fn, slots):
        for _ in range(a.warmup):
            fn()
        wall, ms = [], {k: [] for k in slots}
        for _ in range(a.steps):
            t0 = time.perf_counter()
            fn()
            wall.append(time.perf_counter() - t0)
            for k, slot in slots.items():
                ms[k].append(ctx.kernel_ms(slot))
        c = [int(x) for x in ctx.counters()]
        out = {"tree_steps": c[0], "rows": c[1], "rows_per_step": c[1] / max(1, c[0]), "general_steps": c[3]}
        out.update(mm([w * 1e3 for w in wall], "wall_ms"))
        for k in slots:
            out.update(mm(ms[k], k))
        return out, ms

    def approx_leg(k, chunk_len):
        out, ms = leg(lambda: ctx.approx_run(1, k, 0, 0, chunk_len, a.max_steps), {"run_ms": 6, "exact_ms": 0, "tree_ms": 3})
        both = [x + y for x, y in zip(ms["exact_ms"], ms["tree_ms"])]
        out.update(mm([v * 1e9 / max(1, out["tree_steps"]) for v in both], "ps_per_step"))
        res = ctx.approx_fetch(want_hits=False)[0]
        out.update({"incomplete_share": float((res["complete"] == 0).mean()), "positions": [int(x) for x in res["cnt"].sum(axis=0)], "strings": int(res["n_hits"].sum()),
                    "tasks_with_a_hit": int((res["n_hits"] > 0).sum())})
        return out

    def count_leg():
        out, ms = leg(lambda: ctx.locate_run(1, 0), {"run_ms": 6, "count_kernel_ms": 0})
        out.update(mm([v * 1e9 / max(1, out["tree_steps"]) for v in ms["count_kernel_ms"]], "ps_per_step"))
        return out

    out = {"reads": a.reads, "read_len": a.read_len, "piece": a.piece, "steps": a.steps, "warmup": a.warmup, "max_steps": a.max_steps}
    out["pieces_count"] = count_leg()
    for k in (1, 2):
        for cl in CHUNKS:
            out["pieces_k%d_chunk%d" % (k, cl)] = approx_leg(k, cl)
    ctx.swap(0)                                  # the whole reads resident
    out["reads_count"] = count_leg()
    for cl in CHUNKS:
        out["reads_k1_chunk%d" % cl] = approx_leg(1, cl)
    for name, base in (("pieces_k1", "pieces_count"), ("pieces_k2", "pieces_count"), ("reads_k1", "reads_count")):
        for cl in CHUNKS:
            out["%s_chunk%d_over_count_per_step" % (name, cl)] = out["%s_chunk%d" % (name, cl)]["ps_per_step_median"] / out[base]["ps_per_step_median"]
    print(json.dumps(out))
    ctx.close()
    idx.close()


if __name__ == "__main__":
    main()
