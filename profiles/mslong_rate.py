"""Rate of matching statistics of long patterns (moni_ms_long_batch) on the benchmark's index, beside the one-lane-per-pattern path
(moni_ms_lengths_batch) in the same process and from the same build: one context, 3 warm-up + 10 timed calls per leg, minimum - median - maximum.

  pattern   one haplotype of the benchmark pangenome, --bases long, mutated as the benchmark's reads are (1 % substitutions, 0.05 % indels)
  baseline  moni_ms_lengths_batch on its first --baseline-bases bases (the step-major workspace takes 64 x 8 x 2 bytes per base): time per LF step
            of ms_lf_kernel, which = 0 of moni_last_kernel_ms - one lane walks the pattern (its idle second strand lane walks the reverse complement)
  table     seg_len x overlap: time per LF step of the speculative walk (t_walk / steps_spec), the flagged share, steps_chain, the rounds' times
  chain     the chain round on the pattern, and on a verbatim substring of the text of --baseline-bases bases: every segment flagged, one lane

Prints one JSON line.  The index file must exist (a bench.py run with the same --base-len / --haps writes it); nothing is built here.

    python profiles/mslong_rate.py [--cache DIR] [--base-len N --haps H] [--bases N] [--baseline-bases N] [--steps K] [--warmup W]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEG_LENS = (512, 1024, 4096, 16384)
OVERLAPS = (64, 256, 1024)


def mutated(seq, seed=150, sub_rate=0.01, indel_rate=0.0005):
    """synth.make_reads' errors on one long sequence: single-base insertions and deletions at indel_rate per base, then substitutions at sub_rate"""
    rng = np.random.Generator(np.random.MT19937(seed))
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    at = np.nonzero(rng.random(len(seq)) < indel_rate)[0]
    ins = rng.random(len(at)) < 0.5
    out = np.delete(seq, at[~ins])
    shift = np.searchsorted(at[~ins], at[ins])
    out = np.insert(out, at[ins] - shift, acgt[rng.integers(0, 4, size=int(ins.sum()))])
    code = np.zeros(256, dtype=np.uint8)
    code[acgt] = np.arange(4, dtype=np.uint8)
    sub = rng.random(len(out)) < sub_rate
    return np.where(sub, acgt[(code[out] + rng.integers(1, 4, size=len(out), dtype=np.uint8)) & 3], out)


def spread(v):
    return {"min": float(min(v)), "median": float(np.median(v)), "max": float(max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache", default="/tmp/moni_bench_cache")
    ap.add_argument("--base-len", type=int, default=61420004)
    ap.add_argument("--haps", type=int, default=12)
    ap.add_argument("--bases", type=int, default=16 << 20)
    ap.add_argument("--baseline-bases", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from moni_align_amd import capi, synth
    path = os.path.join(a.cache, "idx_%d_%d_lifted_0.mfi" % (a.base_len, a.haps))
    if not os.path.exists(path):
        sys.exit("no cached index %s: run bench.py with the same --base-len / --haps first" % path)
    pg = synth.make_pangenome(a.base_len, a.haps, seed=19, var_seed=12)
    hap = pg.seqs[min(3, len(pg.seqs) - 1)]
    del pg
    bases = min(a.bases, len(hap) - 1000)
    pat = np.ascontiguousarray(mutated(hap[500:500 + bases]))
    offs = np.array([0, len(pat)], dtype=np.uint64)
    verbatim = np.ascontiguousarray(hap[2000:2000 + a.baseline_bases])
    del hap
    idx = capi.Index(path=path, device=0)
    ctx = capi.Ctx(idx)
    out = {"bases": int(len(pat)), "baseline_bases": a.baseline_bases, "steps": a.steps, "warmup": a.warmup}

    # baseline: one lane per pattern
    bp = pat[:a.baseline_bases]
    bo = np.array([0, len(bp)], dtype=np.uint64)
    walk = []
    _, ln0 = ctx.ms_lengths_batch(bp, bo)
    ctx.upload(bp, bo)
    for k in range(a.warmup + a.steps):
        ctx.ms_run()                                           # device only: pack_kernel + ms_lf_kernel over the resident batch
        if k >= a.warmup:
            walk.append(ctx.kernel_ms(0))
    out["baseline"] = {"walk_ms": spread(walk), "ns_per_lf_step": spread([w * 1e6 / len(bp) for w in walk])}          # strand 0's lane: len(bp) dependent steps

    def leg(seq, o, seg_len, overlap):
        tw, tl, tc, tt = [], [], [], []
        for k in range(a.warmup + a.steps):
            _, ln, st = ctx.ms_long_batch(seq, o, seg_len, overlap, want_pointers=False)
            if k >= a.warmup:
                tw.append(st["t_walk"] * 1e3); tl.append(st["t_len"] * 1e3); tc.append(st["t_chain"] * 1e3); tt.append(st["t_total"] * 1e3)
        return ln, st, {"seg_len": seg_len, "overlap": overlap, "segments": st["segments"], "flagged": st["flagged"], "flagged_share": st["flagged"] / max(1, st["segments"]),
                        "chain_runs": st["chain_runs"], "steps_spec": st["steps_spec"], "steps_chain": st["steps_chain"], "jumps": st["jumps"],
                        "walk_ms": spread(tw), "len_ms": spread(tl), "chain_ms": spread(tc), "total_ms": spread(tt),
                        "ps_per_lf_step": spread([w * 1e9 / st["steps_spec"] for w in tw]),
                        "device_ms_per_mbase": float(np.median(tw) + np.median(tl) + np.median(tc)) / (len(seq) / 1e6)}

    table = []
    for seg_len in SEG_LENS:
        for overlap in OVERLAPS:
            ln, st, row = leg(pat, offs, seg_len, overlap)
            if seg_len == SEG_LENS[0] and overlap == OVERLAPS[0]:
                out["lengths_equal_baseline"] = bool(np.array_equal(ln[:len(bp) // 2], ln0[:len(bp) // 2]))          # (the baseline's pattern ends at baseline_bases: only lengths well before its end compare)
            table.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    out["table"] = table
    base_ns = out["baseline"]["ns_per_lf_step"]["median"]
    for row in table:
        row["baseline_over_walk_per_step"] = base_ns * 1e3 / row["ps_per_lf_step"]["median"]
    # worst case: a verbatim substring of the text, every segment flagged, the chain round is one lane
    p = capi.MslongParamsC()
    capi.lib().moni_mslong_params_default(ctypes.byref(p))
    vo = np.array([0, len(verbatim)], dtype=np.uint64)
    _, st, row = leg(verbatim, vo, p.seg_len, p.overlap)
    row["chain_ns_per_lf_step"] = spread([c * 1e6 / max(1, st["steps_chain"]) for c in (row["chain_ms"]["min"], row["chain_ms"]["median"], row["chain_ms"]["max"])])
    out["verbatim"] = row
    out["defaults"] = {"seg_len": p.seg_len, "overlap": p.overlap}
    print(json.dumps(out))
    ctx.close()
    idx.close()


if __name__ == "__main__":
    main()
