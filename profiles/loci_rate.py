"""Rate of the loci query (moni_loci_run) on the benchmark's index, beside the only other way to the same answer from code it does not touch -
moni_locate_run with max_occ = the batch's largest count, the fetch of its positions, the lift of every position on the host (levioSAM's
lift_pos = ins.rank0(del.select0(p + 1)) over the flat index's ins / del column lists, three numpy.searchsorted calls) and numpy.unique of the
(task, lifted position) pairs - in the same process and from the same build: one context, 3 warm-up steps and 10 timed steps per leg.  Two workloads:
"short", 1 M 32-base pieces of the benchmark's reads (counts about the number of haplotypes), and "skewed", 4096 pieces of 12 bases (counts from none
to a few hundred in one batch).  Per leg: wall time of the call (for the yardstick: run + fetch + lift + unique), the HIP-event time of the whole run, of count_kernel,
of the walk (planning and scans included) and of the sort and fold, their minimum - maximum over the timed steps, the phi steps, the segments, the
loci and the loci per occurrence.  The walk is timed with lift = 0 too (the price of the lift lookups).  The results of the two routes are compared
before anything is timed.  Prints one JSON line.

    python profiles/loci_rate.py [--cache DIR] [--base-len N --haps H] [--reads N] [--steps K] [--warmup W] [--piece L] [--skew-reads N --skew-piece L]

The index file must exist (a bench.py run with the same --base-len / --haps writes it); nothing is built here."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class HostLift:
    """liftidx::lift of arrays of text positions from a flat index's lifts (null lifts: the positions themselves)"""

    def __init__(self, fi):
        self.starts = np.asarray(fi.seq_starts).astype(np.int64)
        self.lf = fi.lifts
        if self.lf is not None:
            n = len(self.starts) - 1
            self.second = np.asarray(self.lf.second).astype(np.int64)
            self.ins = [np.asarray(self.lf.ins_of(i)).astype(np.int64) for i in range(n)]
            # del column k of a sequence has k deleted columns in front of it: the haplotype position that follows it is del[k] - k
            self.del_hap = [np.asarray(self.lf.del_of(i)).astype(np.int64) - np.arange(len(self.lf.del_of(i)), dtype=np.int64) for i in range(n)]

    def __call__(self, pos):
        pos = pos.astype(np.int64)
        if self.lf is None:
            return pos
        sid = np.minimum(np.searchsorted(self.starts, pos, side="right") - 1, len(self.starts) - 2)
        out = np.empty_like(pos)
        for i in np.unique(sid):
            m = sid == i
            ph = pos[m] - self.starts[i]
            x = ph + np.searchsorted(self.del_hap[i], ph, side="right")          # del.select0(ph + 1): the column of haplotype position ph
            out[m] = self.second[i] + x - np.searchsorted(self.ins[i], x, side="left")          # ins.rank0(x)
        return out


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
    from moni_align_amd import capi, index_build, synth
    path = os.path.join(a.cache, "idx_%d_%d_lifted_0.mfi" % (a.base_len, a.haps))
    if not os.path.exists(path):
        sys.exit("no cached index %s: run bench.py with the same --base-len / --haps first" % path)
    pg = synth.make_pangenome(a.base_len, a.haps, seed=19, var_seed=12)
    reads = synth.make_reads(pg, a.reads, a.read_len, seed=150)
    del pg
    host_lift = HostLift(index_build.FlatIndex.load(path, mmap=True))

    def cut(n, piece, seed):
        at = np.random.default_rng(seed).integers(0, a.read_len - piece + 1, size=n)
        p = reads[np.arange(n)[:, None], at[:, None] + np.arange(piece)[None, :]]
        return np.ascontiguousarray(p).reshape(-1), np.arange(0, (n + 1) * piece, piece, dtype=np.uint64)

    idx = capi.Index(path=path, device=0)
    ctx = capi.Ctx(idx)
    mm = lambda v, k: {k + "_median": float(np.median(v)), k + "_min": float(min(v)), k + "_max": float(max(v))}

    def timed(fn, slots):
        for _ in range(a.warmup):
            fn()
        wall, ms = [], {k: [] for k in slots}
        for _ in range(a.steps):
            t0 = time.perf_counter()
            fn()
            wall.append(time.perf_counter() - t0)
            for k, which in slots.items():
                ms[k].append(ctx.kernel_ms(which))
        out = {"phi_steps": int(ctx.counters()[2])}
        out.update(mm([w * 1e3 for w in wall], "wall_ms"))
        for k in slots:
            out.update(mm(ms[k], k))
        return out

    LOCI = {"run_ms": 6, "count_kernel_ms": 0, "walk_ms": 3, "sort_fold_ms": 4}
    LOC = {"run_ms": 6, "count_kernel_ms": 0, "walk_ms": 3}

    def workload(n, piece, seed):
        ctx.upload(*cut(n, piece, seed))
        ctx.loci_run(1, 1, 0, 0)
        res, lpos, lseq, lseq_off, support = ctx.loci_fetch()
        top = int(res["count"].max())

        def yardstick():
            ctx.locate_run(1, top)
            lres, pos, sq, so = ctx.locate_fetch()
            task = np.repeat(np.arange(len(lres), dtype=np.int64), lres["n_occ"])
            key, cnt = np.unique((task << 40) | host_lift(pos), return_counts=True)
            return key, cnt

        key, cnt = yardstick()          # the two routes agree before either is timed
        task = np.repeat(np.arange(len(res), dtype=np.int64), res["n_loci"].astype(np.int64))
        assert np.array_equal(key, (task << 40) | lpos.astype(np.int64)) and np.array_equal(cnt.astype(np.uint64), support)
        occ = int(res["count"].sum())
        out = {"patterns": n, "piece": piece, "max_count": top, "occurrences": occ, "segments": int(res["n_segs"].sum()), "loci": len(lpos),
               "loci_per_occurrence": len(lpos) / max(occ, 1), "patterns_that_occur": int((res["count"] > 0).sum())}
        out["loci_run"] = timed(lambda: ctx.loci_run(1, 1, 0, 0), LOCI)
        out["loci_run_no_lift"] = timed(lambda: ctx.loci_run(1, 0, 0, 0), LOCI)
        out["loci_run_and_fetch"] = timed(lambda: (ctx.loci_run(1, 1, 0, 0), ctx.loci_fetch()), LOCI)
        out["locate_fetch_lift_unique"] = timed(yardstick, LOC)
        out["yardstick_over_loci_wall"] = out["locate_fetch_lift_unique"]["wall_ms_median"] / out["loci_run_and_fetch"]["wall_ms_median"]
        return out

    out = {"steps": a.steps, "warmup": a.warmup}
    out["short"] = workload(a.reads, a.piece, 32)
    out["skewed"] = workload(a.skew_reads, a.skew_piece, 12)
    print(json.dumps(out))
    ctx.close()
    idx.close()


if __name__ == "__main__":
    main()
