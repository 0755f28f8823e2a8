"""Runs of anchors per read, anchors of the longest run, chain starts and kept chains per read - what the caps of chain_runs_kernel (AF_RUN_LEN, 16 run
slots, AF_RUN_CHAINS) have to hold - on a sample of reads drawn the way bench.py draws its batch, over a small pangenome of the same model; seeds by the
CPU oracle, chaining by tests/chain_runs_model.py.  Needs no GPU.  python profiles/chain_runs_hist.py [HAPS [READS]]"""
import os, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from tests import chain_runs_model as T
from moni_align_amd import index_build, synth
from oracle import orc

haps = int(sys.argv[1]) if len(sys.argv) > 1 else 12
n = int(sys.argv[2]) if len(sys.argv) > 2 else 3000
pg = synth.make_pangenome(200000, haps, seed=19, var_seed=12)
fi = index_build.build_from_pangenome(pg, device="cpu")
d = tempfile.mkdtemp(); p = os.path.join(d, "c.mfi"); fi.save(p)
o = orc.OracleIndex(p)
reads = synth.make_reads(pg, n, 150, seed=150)
offs = np.arange(0, (n + 1) * 150, 150, dtype=np.uint64)
w = o.seed_batch(reads.reshape(-1), offs, 25, True, 1000, threads=8)
mems = np.zeros(len(w["pos"]), dtype=[(f, np.uint64) for f in ("pos", "len", "idx", "mate", "rpos", "occ_cnt", "occ_off")])
for f in mems.dtype.names:
    mems[f] = w[f]
ms = T.models(dict(mems=mems, occs=w["occs"], read_mem_off=w["read_mem_off"]))
def hist(key):
    v = np.array([m[key] for m in ms]); return {int(k): int(c) for k, c in zip(*np.unique(v, return_counts=True))}
print("sequences", len(pg.seqs), "reads", n)
print("anchors/read mean", np.mean([m["n"] for m in ms]))
print("runs per read", hist("n_runs"))
print("longest run", hist("max_run"))
rl = np.array([x for m in ms for x in m["run_lens"]]); print("anchors per run", {int(k): int(c) for k, c in zip(*np.unique(rl, return_counts=True))}, "mean %.2f" % rl.mean())
print("kept chains", hist("kept"))
print("starts", hist("starts"))
l0 = [m for m in ms if m["n"] <= 96 and m["seeds"] <= 24]
print("list0", len(l0), "gate", sum(m["gate"] for m in ms), "routed", sum(m["routed"] for m in ms))
for rl in (4, 5, 6, 7, 8, 10, 12, 16):
    print(" RUN_LEN", rl, "covers of list0:", sum(1 for m in l0 if m["n"] > 0 and m["max_run"] <= rl and m["n_runs"] <= 16) / max(1, len(l0)))
