"""Rates of the depth of coverage on the benchmark's workload: the index bench.py caches, one context, the records of the
1 M-read step (moni_align_stream, then moni_bam_sorted_run) as one chunk of the merge, 3 warm-up + 10 timed calls of each leg in one process;
median (min - max) of the library's own figures and of host seconds around the calls.

  add      moni_bam_sort (raw) of the chunk, then moni_cov_add_sorted: t_add beside t_key and t_gather of the same chunk; moni_cov_add of the
           same bytes from host memory (t_add and t_total)
  seal     moni_cov_seal of an object that has taken the chunk once: host seconds, per 10^9 slots
  text     all pieces of moni_cov_next at the front end's limits (64 Mi slots, 4 Mi lines): host seconds, per 10^9 slots and per 10^6 lines
  windows  moni_cov_windows of every reference at --window: host seconds
  frontend moni-hip-align --bam --sort --mark-dup with and without --coverage on the same FASTQ file, one after the other, twice: wall
           seconds, the front end's elapsed seconds, its Coverage line (skipped with --no-frontend)

The depth is checked against a difference array built here with numpy from the sorted records.  Prints one JSON line.

    python profiles/coverage_rate.py [--cache DIR] [--base-len N --haps H] [--reads N] [--steps K] [--warmup W] [--window N] [--no-frontend]

The index file must exist (a bench.py run with the same --base-len / --haps writes it); nothing is built here."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    ap.add_argument("--window", type=int, default=500)
    ap.add_argument("--no-frontend", action="store_true")
    a = ap.parse_args()
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
    header = ctx.sam_header()
    ctx.bam_set_header(header)
    rec, keys, roff, _ = ctx.bam_sorted_run(sam)
    del sam
    n_rec = len(roff) - 1
    recbuf = np.frombuffer(rec, dtype=np.uint8)
    roff = np.ascontiguousarray(roff, dtype=np.uint64)

    # ---- the adds ----
    p = capi.BamParamsC()
    L.moni_bam_params_default(C.byref(p))
    p.raw = 1
    out, on, ents, st, vs = C.c_void_p(), C.c_uint64(), C.c_void_p(), capi.BamSortStatsC(), capi.CovStatsC()
    cov = capi.Coverage(ctx)
    t = {k: [] for k in ("t_key", "t_gather", "t_add_sorted", "t_add_sorted_total", "t_add_host", "t_add_host_total")}
    for k in range(a.warmup + a.steps):
        if L.moni_bam_sort(ctx._h, recbuf.ctypes.data, recbuf.size, roff.ctypes.data, n_rec, C.byref(p), C.byref(out), C.byref(on), C.byref(ents), C.byref(st)):
            sys.exit("moni_bam_sort failed")
        if L.moni_cov_add_sorted(ctx._h, cov._h, C.byref(vs)):
            sys.exit("moni_cov_add_sorted failed")
        sorted_stats = cov._stats(vs)
        if k >= a.warmup:
            t["t_key"].append(st.t_key); t["t_gather"].append(st.t_gather); t["t_add_sorted"].append(vs.t_add); t["t_add_sorted_total"].append(vs.t_total)
        if L.moni_cov_add(ctx._h, cov._h, recbuf.ctypes.data, recbuf.size, roff.ctypes.data, n_rec, C.byref(vs)):
            sys.exit("moni_cov_add failed")
        if k >= a.warmup:
            t["t_add_host"].append(vs.t_add); t["t_add_host_total"].append(vs.t_total)
    cov.close()

    # ---- seal, text, windows: an object that took the chunk once ----
    t_seal, t_text, t_win, pieces = [], [], [], 0
    n_lines = text_bytes = 0
    refs = []
    for k in range(a.warmup + a.steps):
        cov = capi.Coverage(ctx)
        rc, _ = cov.add_sorted(ctx)
        assert rc == 0
        t0 = time.perf_counter()
        rc, refs = cov.seal(ctx)
        t1 = time.perf_counter()
        assert rc == 0
        tx, tn, done = C.c_void_p(), C.c_uint64(), C.c_int(0)
        pieces = n_lines = text_bytes = 0
        spent = 0.0
        while not done.value:
            t2 = time.perf_counter()
            if L.moni_cov_next(ctx._h, cov._h, 64 << 20, 4 << 20, C.byref(tx), C.byref(tn), C.byref(done)):
                sys.exit("moni_cov_next failed")
            spent += time.perf_counter() - t2
            pieces += 1
            text_bytes += tn.value
            if k == a.warmup + a.steps - 1 and tn.value:          # counted outside the timed part, once
                n_lines += int(np.count_nonzero(np.frombuffer((C.c_char * tn.value).from_address(tx.value), dtype=np.uint8) == 10))
        t3 = time.perf_counter()
        for r in range(len(refs)):
            rc, _ = cov.windows(ctx, r, a.window)
            assert rc == 0
        t4 = time.perf_counter()
        if k >= a.warmup:
            t_seal.append(t1 - t0); t_text.append(spent); t_win.append(t4 - t3)
        if k == a.warmup + a.steps - 1:          # the check, on the last object
            lens = [x[0] for x in refs]
            diffs = [np.zeros(ln + 1, np.int32) for ln in lens]
            mv = recbuf
            o = roff.astype(np.int64)

            def field(byte, dtype):
                w = np.dtype(dtype).itemsize
                return np.stack([mv[o[:-1] + byte + j] for j in range(w)], axis=1).copy().view(dtype).reshape(-1)

            ref, pos, nops, flag, lname = field(4, "<i4"), field(8, "<i4"), field(16, "<u2"), field(18, "<u2"), mv[o[:-1] + 12]
            counted = np.flatnonzero((ref >= 0) & (pos >= 0) & (nops > 0) & ((flag & 0x704) == 0))
            for i in counted.tolist():
                at, pp = int(o[i]) + 36 + int(lname[i]), int(pos[i])
                start = pp
                for c in range(int(nops[i])):
                    v = int.from_bytes(mv[at + 4 * c:at + 4 * c + 4].tobytes(), "little")
                    if v & 15 in (0, 2, 7, 8):
                        pp += v >> 4
                    elif v & 15 == 3:
                        if pp > start and start < lens[ref[i]]:
                            diffs[ref[i]][start] += 1; diffs[ref[i]][min(pp, lens[ref[i]])] -= 1
                        pp += v >> 4
                        start = pp
                if pp > start and start < lens[ref[i]]:
                    diffs[ref[i]][start] += 1; diffs[ref[i]][min(pp, lens[ref[i]])] -= 1
            want = []
            for r, ln in enumerate(lens):
                d = np.cumsum(diffs[r], dtype=np.int32)[:-1]
                diffs[r] = None
                want.append((ln, int(d.sum(dtype=np.int64)), int(d.min()), int(d.max())))
            assert want == refs, "the sealed figures differ from the difference array built here"
        cov.close()
    ctx.close()
    idx.close()
    slots = sum(x[0] + 1 for x in refs)
    res = {"steps": a.steps, "warmup": a.warmup, "reads": a.reads, "aligned": ast["aligned"], "records": n_rec, "bam_bytes": int(recbuf.size), "n_ref": len(refs), "slots": slots,
           "stats_of_one_add": {k: v for k, v in sorted_stats.items() if not k.startswith("t_")}, "mean_depth": sum(x[1] for x in refs) / sum(x[0] for x in refs),
           "add": {k + "_ms": spread(v, 1e3) for k, v in t.items()},
           "t_add_over_key_plus_gather": float(np.median(t["t_add_sorted"]) / (np.median(t["t_key"]) + np.median(t["t_gather"]))),
           "seal_s": spread(t_seal), "seal_s_per_Gslot": float(np.median(t_seal)) / slots * 1e9,
           "text": {"pieces": pieces, "lines": n_lines, "bytes": text_bytes, "s": spread(t_text), "s_per_Gslot": float(np.median(t_text)) / slots * 1e9,
                    "s_per_Mline": float(np.median(t_text)) / max(n_lines, 1) * 1e6},
           "windows": {"window": a.window, "s": spread(t_win)}}

    # ---- the front end ----
    if not a.no_frontend:
        fq = "/tmp/coverage_reads.fq"
        synth.write_fastq(fq, reads)
        exe = os.path.join(ROOT, "moni_align_amd", "host", "moni-hip-align")
        fe = []
        for rnd in range(2):
            for extra in ([], ["--coverage", "--cov-window", str(a.window)]):
                o = "/tmp/coverage_fe_%d%s.sam" % (rnd, "_cov" if extra else "")
                t0 = time.time()
                r = subprocess.run([exe, path[:-4], "-p", fq, "-o", o, "-t", "16", "-S", "1000", "-F", "0.5", "--bam", "--sort", "--mark-dup"] + extra, capture_output=True, text=True, timeout=400)
                wall = time.time() - t0
                if r.returncode:
                    sys.exit("the front end failed: " + r.stderr[-2000:])
                el = re.search(r"Elapsed time \(s\): ([0-9.]+)", r.stdout)
                mg = re.search(r"Sorted output: .*", r.stdout)
                cv = re.search(r"Coverage: .*", r.stdout)
                fe.append({"extra": extra, "wall_s": wall, "elapsed_s": float(el.group(1)) if el else None, "merge": mg.group(0) if mg else None, "coverage": cv.group(0) if cv else None,
                           "bam_bytes": os.path.getsize(o[:-4] + ".bam"),
                           "per_base_bytes": os.path.getsize(o[:-4] + ".bam.per-base.bed.gz") if extra else 0, "regions_bytes": os.path.getsize(o[:-4] + ".bam.regions.bed.gz") if extra else 0})
        res["frontend"] = fe
    print(json.dumps(res))


if __name__ == "__main__":
    main()
