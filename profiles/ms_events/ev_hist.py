"""Events per task on the benchmark's batch (configs[2]: 1 M x 150 bp reads, seed 150, the cached index of bench.py): how many 64-byte lines the walk of
the seeding stage writes per task.  The library keeps the lists on the device, so the counts are taken from the dense pointers of moni_ms_query_batch,
chunk by chunk: one event for the start and one wherever a pointer is not its right neighbour's minus one (a lower bound that misses only a jump onto
exactly that value; its sum is checked against the walk's own jump counter).  "Live" stands for the tasks that hold a MEM of 25 bases (moni_seed_run):
the strand prefilter keeps those and a few more.  usage: python3 profiles/ms_events/ev_hist.py [reads]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from moni_align_amd import capi, index_build, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
L, CHUNK = 150, 100000
pg = synth.make_pangenome(61420004, 12, seed=19, var_seed=12)
reads = synth.make_reads(pg, N, L, seed=150)
fi = index_build.FlatIndex.load("/tmp/moni_bench_cache/idx_61420004_12_lifted_0.mfi", mmap=True)
idx = capi.Index(fi=fi, device=0)
ctx = capi.Ctx(idx)
counts = np.zeros((N, 2), dtype=np.int64)
has_mem = np.zeros((N, 2), dtype=bool)
jumps = 0
for lo in range(0, N, CHUNK):
    part = reads[lo:lo + CHUNK]
    offs = np.arange(0, (len(part) + 1) * L, L, dtype=np.uint64)
    p = ctx.ms_query_batch(part.reshape(-1), offs).reshape(len(part), 2, L)
    jumps += int(ctx.counters()[1])
    counts[lo:lo + len(part)] = 1 + np.count_nonzero(p[:, :, :-1] + np.uint64(1) != p[:, :, 1:], axis=2)
    ctx.upload(part.reshape(-1), offs)
    ctx.seed_run(25, True, 1000)
    m = ctx.seed_fetch()["mems"]
    has_mem[lo + m["read"].astype(np.int64), (m["mate"] // 2).astype(np.int64)] = True


def report(name, c):
    h = np.bincount(c)
    print("%s: %d tasks, %d events, mean %.2f, median %d, max %d; share above 8: %.3f, above 16: %.3f, above 32: %.3f; 64-byte lines per task: %.2f" %
          (name, len(c), int(c.sum()), c.mean(), int(np.median(c)), int(c.max()), (c > 8).mean(), (c > 16).mean(), (c > 32).mean(), ((c + 7) // 8).mean()))
    print("  events:tasks " + " ".join("%d:%d" % (k, v) for k, v in enumerate(h) if v))


print("%d reads of %d bases; the walks' jump counter: %d, events counted from the pointers minus one start each: %d" % (N, L, jumps, int(counts.sum()) - 2 * N))
report("tasks that hold a MEM", counts[has_mem])
report("tasks without one", counts[~has_mem])
report("all tasks", counts.reshape(-1))
ctx.close()
idx.close()
