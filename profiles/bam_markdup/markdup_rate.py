"""Cost of duplicate marking on the benchmark's workload, by the method of profiles/bam_sort_rate.py: the index bench.py caches, one
context, the SAM text of the 1 M-read step in pinned memory, 3 warm-up + 10 timed calls of each leg in one process; median (min - max) of the
library's own figures.

  run          moni_bam_sorted_run beside moni_bam_sorted_run_dup (paired = 0) on the same text: t_total of both, t_sig and t_entry
  resolve      moni_bam_dup_resolve over the run's fragments in four runs, and over half as many pairs made of neighbouring fragments
  sort_chunk   moni_bam_sort beside moni_bam_sort_marked (a tenth of the marks set) on the first --chunk bytes (256 MiB) of the records
  frontend     moni-hip-align --bam --sort without and with --mark-dup on the same FASTQ file, one after the other, twice (skipped with --no-frontend)

Prints one JSON line.  The index file must exist (a bench.py run with the same --base-len / --haps writes it); nothing is built here.

    python profiles/bam_markdup/markdup_rate.py [--cache DIR] [--base-len N --haps H] [--reads N] [--steps K] [--warmup W] [--chunk BYTES] [--no-frontend]"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def spread(v, scale=1.0):
    return {"median": float(np.median(v)) * scale, "min": min(v) * scale, "max": max(v) * scale}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache", default="/tmp/moni_bench_cache")
    ap.add_argument("--base-len", type=int, default=61420004)
    ap.add_argument("--haps", type=int, default=12)
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=256 << 20)
    ap.add_argument("--no-frontend", action="store_true")
    a = ap.parse_args()
    import torch
    from moni_align_amd import capi, synth
    path = os.path.join(a.cache, "idx_%d_%d_lifted_0.mfi" % (a.base_len, a.haps))
    if not os.path.exists(path):
        sys.exit("no cached index %s: run bench.py with the same --base-len / --haps first" % path)
    pg = synth.make_pangenome(a.base_len, a.haps, seed=19, var_seed=12)
    reads = synth.make_reads(pg, a.reads, a.read_len, seed=150)
    del pg
    offs = np.arange(0, (a.reads + 1) * a.read_len, a.read_len, dtype=np.uint64)
    names, noff = synth.make_names(a.reads)
    quals = np.full(reads.size, ord("I"), dtype=np.uint8)
    idx = capi.Index(path=path, device=0)
    ctx = capi.Ctx(idx)
    L = capi.lib()
    sam, ast = ctx.align_batch(reads.reshape(-1), offs, names, noff, quals, stream=True)
    n = len(sam)
    pinned = torch.frombuffer(bytearray(sam), dtype=torch.uint8).pin_memory()
    ctx.bam_set_header(ctx.sam_header())
    rounds = range(a.warmup + a.steps)

    # ---- the run, without and with its entries ----
    rec, rl, keys, roff, nr, st = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_void_p(), C.c_uint64(), capi.BamSortStatsC()
    dups, nd, ds = C.c_void_p(), C.c_uint64(), capi.BamRunDupStatsC()
    plain, with_dup, legs = [], [], {k: [] for k in ("t_sig", "t_entry")}
    for k in rounds:
        if L.moni_bam_sorted_run(ctx._h, pinned.data_ptr(), n, C.byref(rec), C.byref(rl), C.byref(keys), C.byref(roff), C.byref(nr), C.byref(st)):
            sys.exit("moni_bam_sorted_run failed")
        if L.moni_bam_sorted_run_dup(ctx._h, pinned.data_ptr(), n, 0, C.byref(rec), C.byref(rl), C.byref(keys), C.byref(roff), C.byref(nr), C.byref(dups), C.byref(nd), C.byref(ds)):
            sys.exit("moni_bam_sorted_run_dup failed")
        if k >= a.warmup:
            plain.append(st.t_total); with_dup.append(ds.run.t_total)
            for f in legs:
                legs[f].append(getattr(ds, f))
    n_rec, bam_bytes, n_ent = nr.value, rl.value, nd.value
    records = np.frombuffer(C.string_at(rec.value, bam_bytes), dtype=np.uint8)
    rec_off = np.frombuffer(C.string_at(roff.value, 8 * (n_rec + 1)), dtype=np.uint64).copy()
    ents = np.frombuffer(C.string_at(dups.value, capi.BAM_DUP_DTYPE.itemsize * n_ent), dtype=capi.BAM_DUP_DTYPE).copy()
    res = {"steps": a.steps, "warmup": a.warmup, "reads": a.reads, "aligned": ast["aligned"], "records": n_rec, "bam_bytes": bam_bytes, "entries": n_ent,
           "run": {"sorted_run_t_total_ms": spread(plain, 1e3), "sorted_run_dup_t_total_ms": spread(with_dup, 1e3), "t_sig_ms": spread(legs["t_sig"], 1e3),
                   "t_entry_ms": spread(legs["t_entry"], 1e3)}}

    # ---- the resolve: the fragments in four runs; half as many pairs of neighbouring fragments ----
    def resolve(runs, n_records, what):
        t = {k: [] for k in ("t_sort", "t_flag", "t_total")}
        for k in rounds:
            marks, s = ctx.bam_dup_resolve(runs, n_records)
            if k >= a.warmup:
                for f in t:
                    t[f].append(s[f])
        res[what] = dict({f + "_ms": spread(v, 1e3) for f, v in t.items()}, **{f: s[f] for f in ("entries", "pairs", "dup_pairs", "fragments", "dup_fragments", "marked_records")})
        return marks
    resolve([ents], [n_rec], "resolve_fragments_one_run")
    cut = [len(ents) * r // 4 for r in range(5)]
    four = [ents[cut[r]:cut[r + 1]] for r in range(4)]          # the places stay inside [0, n_rec): every run is given n_rec records
    resolve(four, [n_rec] * 4, "resolve_fragments_four_runs")
    half = len(ents) // 2
    pairs = np.zeros(half, capi.BAM_DUP_DTYPE)
    x, y = ents[0:2 * half:2], ents[1:2 * half:2]
    pairs["k1"], pairs["k2"] = np.minimum(x["k1"], y["k1"]), np.maximum(x["k1"], y["k1"])
    pairs["score"], pairs["kind"] = x["score"] + y["score"], 1
    pairs["idx"][:, 0], pairs["idx"][:, 1] = x["idx"][:, 0], y["idx"][:, 0]
    resolve([pairs], [n_rec], "resolve_pairs")
    marks = resolve([ents], [n_rec], "resolve_fragments_one_run")[0]

    # ---- one chunk of the merge, without and with marks ----
    m = int(np.searchsorted(rec_off, a.chunk, side="right")) - 1
    chunk_len = int(rec_off[m])
    cbuf = torch.frombuffer(bytearray(records[:chunk_len].tobytes()), dtype=torch.uint8).pin_memory()
    coff = rec_off[:m + 1].copy()
    cm = np.zeros(m, np.uint8)
    cm[::10] = 1
    p = capi.BamParamsC()
    L.moni_bam_params_default(C.byref(p))
    out, on, e = C.c_void_p(), C.c_uint64(), C.c_void_p()
    chunk = {}
    for what, mk in (("sort", None), ("sort_marked", cm.ctypes.data)):
        t = {k: [] for k in ("t_key", "t_sort", "t_gather", "t_deflate", "t_total")}
        for k in rounds:
            if L.moni_bam_sort_marked(ctx._h, cbuf.data_ptr(), chunk_len, coff.ctypes.data, m, mk, C.byref(p), C.byref(out), C.byref(on), C.byref(e), C.byref(st)):
                sys.exit("moni_bam_sort_marked failed")
            if k >= a.warmup:
                for f in t:
                    t[f].append(getattr(st, f))
        chunk[what] = {f + "_ms": spread(v, 1e3) for f, v in t.items()}
    res["sort_chunk"] = dict(chunk, records=m, bytes=chunk_len, marked=int(cm.sum()), marks_of_the_run=int(marks.sum()))
    ctx.close()
    idx.close()

    # ---- the front end ----
    if not a.no_frontend:
        fq = "/tmp/bam_markdup_reads.fq"
        synth.write_fastq(fq, reads)
        exe = os.path.join(ROOT, "moni_align_amd", "host", "moni-hip-align")
        fe = []
        for rnd in range(2):
            for extra in ([], ["--mark-dup"]):
                o = "/tmp/bam_markdup_fe_%d%s.sam" % (rnd, "_marked" if extra else "")
                t0 = time.time()
                r = subprocess.run([exe, path[:-4], "-p", fq, "-o", o, "-t", "16", "-S", "1000", "-F", "0.5", "--bam", "--sort"] + extra, capture_output=True, text=True, timeout=400)
                wall = time.time() - t0
                if r.returncode:
                    sys.exit("the front end failed: " + r.stderr[-2000:])
                el = re.search(r"Elapsed time \(s\): ([0-9.]+)", r.stdout)
                mg = re.search(r"Sorted output: .*", r.stdout)
                du = re.search(r"Duplicates: .*", r.stdout)
                fe.append({"extra": extra, "wall_s": wall, "elapsed_s": float(el.group(1)) if el else None, "merge": mg.group(0) if mg else None,
                           "duplicates": du.group(0) if du else None, "bam_bytes": os.path.getsize(o[:-4] + ".bam")})
        res["frontend"] = fe
    print(json.dumps(res))


if __name__ == "__main__":
    main()
