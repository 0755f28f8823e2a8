"""Rate and size of the BAM writer (moni_bam_records) on the benchmark's workload, beside the BGZF writer on the same text: the index bench.py
caches, one context, the SAM text of the 1 M-read step (moni_align_stream) in pinned memory, 3 warm-up + 10 timed calls of each in one process;
median (min - max) of the library's own figures - for moni_bam_records t_encode (HIP events from the first newline pass to the write pass,
the two host synchronisations between them included), t_deflate (the block kernel, the scan, the gather) and t_total (the call, with the
upload of the text and the download of the blocks); for the unchanged moni_bgzf_compress t_kernel and t_total.  The BAM stream is read back
by tests/bam_model.decode on the first lines as a check.  Prints one JSON line.

    python profiles/bam_rate.py [--cache DIR] [--base-len N --haps H] [--reads N] [--steps K] [--warmup W]

The index file must exist (a bench.py run with the same --base-len / --haps writes it); nothing is built here."""
import argparse
import ctypes as C
import gzip
import json
import os
import sys

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
    a = ap.parse_args()
    import torch
    from moni_align_amd import capi, synth
    from tests import bam_model
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
    bam_header = ctx.bam_set_header(header)

    def bam_leg(raw):
        p = capi.BamParamsC()
        L.moni_bam_params_default(C.byref(p))
        p.raw = 1 if raw else 0
        out, on, st = C.c_void_p(), C.c_uint64(), capi.BamStatsC()
        te, td, tt = [], [], []
        for k in range(a.warmup + a.steps):
            rc = L.moni_bam_records(ctx._h, pinned.data_ptr(), n, C.byref(p), C.byref(out), C.byref(on), C.byref(st))
            if rc:
                sys.exit("moni_bam_records failed with code %d (bad lines %d, first %d, reason %d)" % (rc, st.bad_lines, st.first_bad_line, st.bad_reason))
            if k >= a.warmup:
                te.append(st.t_encode); td.append(st.t_deflate); tt.append(st.t_total)
        stats = {k: getattr(st, k) for k, _ in capi.BamStatsC._fields_ if not k.startswith("t_") and k != "pad"}
        return C.string_at(out.value, on.value), stats, {"t_encode_ms": spread(te, 1e3), "t_deflate_ms": spread(td, 1e3), "t_total_ms": spread(tt, 1e3)}

    def bgzf_leg():
        p = capi.BgzfParamsC()
        L.moni_bgzf_params_default(C.byref(p))
        out, on, st = C.c_void_p(), C.c_uint64(), capi.BgzfStatsC()
        tk, tt = [], []
        for k in range(a.warmup + a.steps):
            rc = L.moni_bgzf_compress(ctx._h, pinned.data_ptr(), n, C.byref(p), C.byref(out), C.byref(on), C.byref(st))
            if rc:
                sys.exit("moni_bgzf_compress failed with code %d" % rc)
            if k >= a.warmup:
                tk.append(st.t_kernel); tt.append(st.t_total)
        return on.value, {"t_kernel_ms": spread(tk, 1e3), "t_total_ms": spread(tt, 1e3)}

    z, stats, t_bam = bam_leg(False)
    raw, _, t_raw = bam_leg(True)
    sam_z_bytes, t_bgzf = bgzf_leg()
    assert gzip.decompress(z) == raw and len(raw) == stats["bam_bytes"]
    # the first records read back by the strict reader
    head = sam[:sam.index(b"\n", 1 << 20) + 1]
    want = bam_model.encode_records(header, head)
    assert raw[:len(want)] == want and bam_model.decode(bam_header + raw[:len(want)]) == header + bam_model.canonical(head)
    enc = t_bam["t_encode_ms"]["median"] * 1e-3
    print(json.dumps({
        "steps": a.steps, "warmup": a.warmup, "reads": a.reads, "aligned": ast["aligned"], "sam_bytes": n, "bytes_per_read": n / a.reads, **stats,
        "bam_over_sam": stats["bam_bytes"] / n, "bam_records": t_bam, "bam_records_raw": t_raw, "bgzf_compress_of_the_sam_text": t_bgzf,
        "compressed_sam_bytes": sam_z_bytes, "compressed_bam_over_compressed_sam": stats["out_bytes"] / sam_z_bytes,
        "compressed_bam_over_bam": stats["out_bytes"] / stats["bam_bytes"], "compressed_sam_over_sam": sam_z_bytes / n,
        "encode_GB_per_s_in": n / enc / 1e9, "encode_GB_per_s_in_plus_out": (n + stats["bam_bytes"]) / enc / 1e9,
        "deflate_ms_per_GB_bam": t_bam["t_deflate_ms"]["median"] / (stats["bam_bytes"] / 1e9), "deflate_ms_per_GB_sam": t_bgzf["t_kernel_ms"]["median"] / (n / 1e9)}))
    ctx.close()
    idx.close()


if __name__ == "__main__":
    main()
