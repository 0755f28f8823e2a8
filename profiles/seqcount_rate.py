"""Rate of the sequence-count query (moni_seqcount_run) on the benchmark's index, beside the only other way to the same table from code it does
not touch - moni_locate_run with max_occ = the batch's largest count, the fetch of its lists and numpy.bincount - in the same process and from
the same build: one context, 3 warm-up steps and 10 timed steps per leg.  Two workloads: "short", 1 M 32-base pieces of the benchmark's reads
(counts about the number of haplotypes), and "skewed", 4096 pieces of 12 bases (counts into the thousands).  Per leg: wall time of the call (for
the yardstick: run + fetch + bincount), the HIP-event time of the whole run, of count_kernel and of the walk, their minimum - maximum over the
timed steps, the phi steps and the segments.  The tables of the two routes are compared before anything is timed.  Prints one JSON line.

    python profiles/seqcount_rate.py [--cache DIR] [--base-len N --haps H] [--reads N] [--steps K] [--warmup W] [--piece L] [--skew-reads N --skew-piece L]

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
    ap.add_argument("--skew-reads", type=int, default=4096)
    ap.add_argument("--skew-piece", type=int, default=12)
    a = ap.parse_args()
    from moni_align_amd import capi, synth
    path = os.path.join(a.cache, "idx_%d_%d_lifted_0.mfi" % (a.base_len, a.haps))
    if not os.path.exists(path):
        sys.exit("no cached index %s: run bench.py with the same --base-len / --haps first" % path)
    pg = synth.make_pangenome(a.base_len, a.haps, seed=19, var_seed=12)
    reads = synth.make_reads(pg, a.reads, a.read_len, seed=150)
    del pg

    def cut(n, piece, seed):
        at = np.random.default_rng(seed).integers(0, a.read_len - piece + 1, size=n)
        p = reads[np.arange(n)[:, None], at[:, None] + np.arange(piece)[None, :]]
        return np.ascontiguousarray(p).reshape(-1), np.arange(0, (n + 1) * piece, piece, dtype=np.uint64)

    idx = capi.Index(path=path, device=0)
    ctx = capi.Ctx(idx)
    mm = lambda v, k: {k + "_median": float(np.median(v)), k + "_min": float(min(v)), k + "_max": float(max(v))}

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        wall, run_ms, count_ms, walk_ms = [], [], [], []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            fn()
            wall.append(time.perf_counter() - t0)
            run_ms.append(ctx.kernel_ms(6))
            count_ms.append(ctx.kernel_ms(0))
            walk_ms.append(ctx.kernel_ms(3))
        out = {"phi_steps": int(ctx.counters()[2])}
        out.update(mm([w * 1e3 for w in wall], "wall_ms"))
        out.update(mm(run_ms, "run_ms"))
        out.update(mm(count_ms, "count_kernel_ms"))
        out.update(mm(walk_ms, "walk_ms"))
        return out

    def workload(n, piece, seed):
        ctx.upload(*cut(n, piece, seed))
        ctx.seqcount_run(1, 0)
        res, counts = ctx.seqcount_fetch()
        n_seq = counts.shape[1]
        top = int(res["count"].max())

        def yardstick():
            ctx.locate_run(1, top)
            lres, pos, sq, so = ctx.locate_fetch()
            task = np.repeat(np.arange(len(lres)), lres["n_occ"])
            return np.bincount(task * n_seq + sq, minlength=len(lres) * n_seq).reshape(len(lres), n_seq)

        assert np.array_equal(yardstick().astype(np.uint64), counts)          # the two routes agree before either is timed
        out = {"patterns": n, "piece": piece, "n_seq": n_seq, "max_count": top, "occurrences": int(res["count"].sum()), "segments": int(res["n_segs"].sum()),
               "patterns_that_occur": int((res["count"] > 0).sum())}
        out["seqcount_run"] = timed(lambda: ctx.seqcount_run(1, 0))
        out["seqcount_run_and_fetch"] = timed(lambda: (ctx.seqcount_run(1, 0), ctx.seqcount_fetch()))
        out["locate_fetch_bincount"] = timed(yardstick)
        out["yardstick_over_seqcount_wall"] = out["locate_fetch_bincount"]["wall_ms_median"] / out["seqcount_run_and_fetch"]["wall_ms_median"]
        return out

    out = {"steps": a.steps, "warmup": a.warmup}
    out["short"] = workload(a.reads, a.piece, 32)
    out["skewed"] = workload(a.skew_reads, a.skew_piece, 12)
    print(json.dumps(out))
    ctx.close()
    idx.close()


if __name__ == "__main__":
    main()
