"""Rate of the coordinate sort of BAM records on the benchmark's workload: the index bench.py caches, one context, the SAM text of the
1 M-read step (moni_align_stream) in pinned memory, 3 warm-up + 10 timed calls of each leg in one process; median (min - max) of the library's own
figures.

  sorted_run   moni_bam_sorted_run beside moni_bam_records with raw = 1 on the same text: t_total of both, and t_key / t_sort / t_gather
  copy         a device-to-device copy (hipMemcpyAsync through torch) of as many bytes as the gather moves, timed by HIP events in the same run
  sort_chunk   moni_bam_sort of the first --chunk bytes (256 MiB) of the records in input order, with the deflater and with raw = 1
  frontend     moni-hip-align --bam and --bam --sort on the same FASTQ file (the same reads), one after the other, twice; wall seconds, the
               front end's own elapsed seconds and what its merge reports (skipped with --no-frontend)

The sorted run is checked against a stable argsort of the keys computed here from the unsorted records.  Prints one JSON line.

    python profiles/bam_sort_rate.py [--cache DIR] [--base-len N --haps H] [--reads N] [--steps K] [--warmup W] [--chunk BYTES] [--no-frontend]

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
    header = ctx.sam_header()
    ctx.bam_set_header(header)
    n_ref = header.count(b"@SQ\t")

    # ---- moni_bam_records raw beside moni_bam_sorted_run ----
    p = capi.BamParamsC()
    L.moni_bam_params_default(C.byref(p))
    p.raw = 1
    out, on, bst = C.c_void_p(), C.c_uint64(), capi.BamStatsC()
    t_raw = []
    for k in range(a.warmup + a.steps):
        if L.moni_bam_records(ctx._h, pinned.data_ptr(), n, C.byref(p), C.byref(out), C.byref(on), C.byref(bst)):
            sys.exit("moni_bam_records failed")
        if k >= a.warmup:
            t_raw.append(bst.t_total)
    unsorted = np.frombuffer(C.string_at(out.value, on.value), dtype=np.uint8)
    rec, rl, keys, roff, nr, st = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_void_p(), C.c_uint64(), capi.BamSortStatsC()
    legs = {k: [] for k in ("t_encode", "t_key", "t_sort", "t_gather", "t_total")}
    for k in range(a.warmup + a.steps):
        if L.moni_bam_sorted_run(ctx._h, pinned.data_ptr(), n, C.byref(rec), C.byref(rl), C.byref(keys), C.byref(roff), C.byref(nr), C.byref(st)):
            sys.exit("moni_bam_sorted_run failed")
        if k >= a.warmup:
            for f in legs:
                legs[f].append(getattr(st, f))
    n_rec, bam_bytes = nr.value, rl.value
    got = np.frombuffer(C.string_at(rec.value, bam_bytes), dtype=np.uint8)
    got_keys = np.frombuffer(C.string_at(keys.value, 8 * n_rec), dtype=np.uint64)
    got_off = np.frombuffer(C.string_at(roff.value, 8 * (n_rec + 1)), dtype=np.uint64)
    # the check: offsets of the unsorted records by their block_size fields, keys from their fields, a stable argsort, the sizes in that order
    uoff = np.zeros(n_rec + 1, dtype=np.int64)
    at = 0
    mv = memoryview(unsorted)
    for i in range(n_rec):
        at += 4 + int.from_bytes(mv[at:at + 4], "little")
        uoff[i + 1] = at
    assert at == bam_bytes == len(unsorted)

    def field(byte, dtype):
        w = np.dtype(dtype).itemsize
        return np.stack([unsorted[uoff[:-1] + byte + j] for j in range(w)], axis=1).copy().view(dtype).reshape(-1)

    ref, pos, flag = field(4, "<i4").astype(np.int64), field(8, "<i4").astype(np.int64), field(18, "<u2").astype(np.int64)
    want_keys = (np.where(ref < 0, n_ref, ref) << 33 | (pos + 1) << 1 | (flag >> 4 & 1)).astype(np.uint64)
    order = np.argsort(want_keys, kind="stable")
    assert np.array_equal(got_keys, want_keys[order]) and np.array_equal(np.diff(got_off.astype(np.int64)), np.diff(uoff)[order])
    for i in (0, 1, n_rec // 2, n_rec - 1):          # the bytes of a few records
        assert np.array_equal(got[int(got_off[i]):int(got_off[i + 1])], unsorted[uoff[order[i]]:uoff[order[i] + 1]])

    # ---- the same bytes through a device-to-device copy ----
    da, db = torch.empty(bam_bytes, dtype=torch.uint8, device="cuda"), torch.empty(bam_bytes, dtype=torch.uint8, device="cuda")
    da.random_(0, 256)
    t_copy = []
    for k in range(a.warmup + a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); db.copy_(da); e1.record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            t_copy.append(e0.elapsed_time(e1) * 1e-3)
    del da, db

    # ---- moni_bam_sort of one chunk ----
    m = int(np.searchsorted(uoff, a.chunk, side="right")) - 1
    chunk_len = int(uoff[m])
    cbuf = torch.frombuffer(bytearray(unsorted[:chunk_len].tobytes()), dtype=torch.uint8).pin_memory()
    coff = uoff[:m + 1].astype(np.uint64)
    chunk = {}
    for raw in (0, 1):
        p.raw = raw
        ents, t = C.c_void_p(), {k: [] for k in ("t_key", "t_sort", "t_gather", "t_deflate", "t_total")}
        for k in range(a.warmup + a.steps):
            if L.moni_bam_sort(ctx._h, cbuf.data_ptr(), chunk_len, coff.ctypes.data, m, C.byref(p), C.byref(out), C.byref(on), C.byref(ents), C.byref(st)):
                sys.exit("moni_bam_sort failed")
            if k >= a.warmup:
                for f in t:
                    t[f].append(getattr(st, f))
        chunk["raw" if raw else "deflated"] = dict({f + "_ms": spread(v, 1e3) for f, v in t.items()}, out_bytes=on.value)
    ctx.close()
    idx.close()

    res = {"steps": a.steps, "warmup": a.warmup, "reads": a.reads, "aligned": ast["aligned"], "sam_bytes": n, "records": n_rec, "bam_bytes": bam_bytes,
           "bytes_per_record": bam_bytes / n_rec, "n_ref": n_ref, "key_bits": 33 + int(n_ref).bit_length(),
           "bam_records_raw_t_total_ms": spread(t_raw, 1e3), "sorted_run": {f + "_ms": spread(v, 1e3) for f, v in legs.items()},
           "d2d_copy_ms": spread(t_copy, 1e3), "gather_over_copy": float(np.median(legs["t_gather"]) / np.median(t_copy)),
           "gather_GB_per_s_read_plus_written": 2 * bam_bytes / float(np.median(legs["t_gather"])) / 1e9,
           "copy_GB_per_s_read_plus_written": 2 * bam_bytes / float(np.median(t_copy)) / 1e9,
           "sort_chunk": dict(chunk, records=m, bytes=chunk_len)}

    # ---- the front end ----
    if not a.no_frontend:
        fq = "/tmp/bam_sort_reads.fq"
        synth.write_fastq(fq, reads)
        exe = os.path.join(ROOT, "moni_align_amd", "host", "moni-hip-align")
        fe = []
        for rnd in range(2):
            for extra in ([], ["--sort"]):
                o = "/tmp/bam_sort_fe_%d%s.sam" % (rnd, "_sorted" if extra else "")
                t0 = time.time()
                r = subprocess.run([exe, path[:-4], "-p", fq, "-o", o, "-t", "16", "-S", "1000", "-F", "0.5", "--bam"] + extra, capture_output=True, text=True, timeout=400)
                wall = time.time() - t0
                if r.returncode:
                    sys.exit("the front end failed: " + r.stderr[-2000:])
                el = re.search(r"Elapsed time \(s\): ([0-9.]+)", r.stdout)
                mg = re.search(r"Sorted output: .*", r.stdout)
                fe.append({"extra": extra, "wall_s": wall, "elapsed_s": float(el.group(1)) if el else None, "merge": mg.group(0) if mg else None,
                           "bam_bytes": os.path.getsize(o[:-4] + ".bam"), "bai_bytes": os.path.getsize(o[:-4] + ".bam.bai") if extra else 0})
        res["frontend"] = fe
    print(json.dumps(res))


if __name__ == "__main__":
    main()
