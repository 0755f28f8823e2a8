"""Rate and ratio of the BGZF writer (moni_bgzf_compress) on the benchmark's workload: the index bench.py caches, one context, the SAM text of the
1 M-read step (moni_align_stream), 3 warm-up + 10 timed calls; median (min - max) of the library's own figures - t_kernel (HIP events: the
per-block kernel, the scan, the gather) and t_total (with the upload of the text and the download of the stream) - for the text in pinned
memory (the intended caller) and in pageable memory.  Yardsticks from the same process: the align step itself, and zlib level 1 on one host
core over the same 65280-byte blocks (x 16: what sixteen such cores would do).  Ratios against zlib level 1 and level 6 cut the same way, for
the benchmark's constant qualities and for quality strings drawn from a binned Phred distribution.  Prints one JSON line.

    python profiles/bgzf_rate.py [--cache DIR] [--base-len N --haps H] [--reads N] [--steps K] [--warmup W] [--zlib-mb M]

The index file must exist (a bench.py run with the same --base-len / --haps writes it); nothing is built here."""
import argparse
import ctypes as C
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BS = 65280


def spread(v, scale=1.0):
    return {"median": float(np.median(v)) * scale, "min": min(v) * scale, "max": max(v) * scale}


def zlib_blocks(data: bytes, level: int):
    """framed size and host seconds of zlib over the blocks of `data` (raw DEFLATE + the 26 bytes BGZF adds per block)"""
    t0 = time.perf_counter()
    n = 0
    for at in range(0, len(data), BS):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        n += len(c.compress(data[at:at + BS])) + len(c.flush()) + 26
    return n, time.perf_counter() - t0


def realistic_quals(n_reads: int, read_len: int, seed: int) -> np.ndarray:
    """binned Phred values (2, 11, 25, 37 as '#', ',', ':', 'F'), the low ones more frequent toward the read's end and clustered in runs"""
    rng = np.random.default_rng(seed)
    pos = np.arange(read_len) / read_len
    p_low = 0.02 + 0.25 * pos ** 3                       # a position's chance to start a run below 37
    start = rng.random((n_reads, read_len)) < p_low / 4
    level = np.where(start, rng.choice(np.array([35, 44, 58], dtype=np.uint8), size=(n_reads, read_len), p=[0.1, 0.35, 0.55]), 0).astype(np.uint8)
    for k in range(1, 4):                                # runs of up to four
        keep = rng.random((n_reads, read_len - k)) < 0.6
        level[:, k:] = np.where((level[:, k:] == 0) & keep, level[:, :-k], level[:, k:])
    return np.where(level == 0, np.uint8(70), level).astype(np.uint8).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache", default="/tmp/moni_bench_cache")
    ap.add_argument("--base-len", type=int, default=61420004)
    ap.add_argument("--haps", type=int, default=12)
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--zlib-mb", type=int, default=64, help="megabytes of the text the host's zlib legs take (the whole text at level 6 takes a quarter of a minute)")
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
    idx = capi.Index(path=path, device=0)
    ctx = capi.Ctx(idx)
    L = capi.lib()

    def align(quals):
        for _ in range(2):
            ctx.align_batch(reads.reshape(-1), offs, names, noff, quals, stream=True, want_text=False)
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            ctx.align_batch(reads.reshape(-1), offs, names, noff, quals, stream=True, want_text=False)
            t.append(time.perf_counter() - t0)
        sam, st = ctx.align_batch(reads.reshape(-1), offs, names, noff, quals, stream=True)
        return sam, spread(t, 1e3), st

    def compress_leg(ptr, n):
        p = capi.BgzfParamsC()
        L.moni_bgzf_params_default(C.byref(p))
        p.eof = 1
        out, on, st = C.c_void_p(), C.c_uint64(), capi.BgzfStatsC()
        tk, tt = [], []
        for k in range(a.warmup + a.steps):
            rc = L.moni_bgzf_compress(ctx._h, ptr, n, C.byref(p), C.byref(out), C.byref(on), C.byref(st))
            if rc:
                sys.exit("moni_bgzf_compress failed with code %d" % rc)
            if k >= a.warmup:
                tk.append(st.t_kernel); tt.append(st.t_total)
        z = C.string_at(out.value, on.value)
        stats = {k: getattr(st, k) for k, _ in capi.BgzfStatsC._fields_ if not k.startswith("t_")}
        return z, stats, {"t_kernel_ms": spread(tk, 1e3), "t_total_ms": spread(tt, 1e3), "transfers_ms": spread([x - y for x, y in zip(tt, tk)], 1e3),
                          "kernel_GB_per_s": n / float(np.median(tk)) / 1e9, "total_GB_per_s": n / float(np.median(tt)) / 1e9}

    def leg(quals, what):
        sam, align_ms, ast = align(quals)
        n = len(sam)
        pinned = torch.frombuffer(bytearray(sam), dtype=torch.uint8).pin_memory()
        z, stats, t_pinned = compress_leg(pinned.data_ptr(), n)
        buf = np.frombuffer(sam, dtype=np.uint8)
        z2, _, t_pageable = compress_leg(buf.ctypes.data, n)
        assert z == z2
        import gzip
        assert gzip.decompress(z) == sam
        part = sam[:min(n, a.zlib_mb << 20) // BS * BS] or sam
        z1_n, z1_s = zlib_blocks(part, 1)
        z6_n, z6_s = zlib_blocks(part, 6)
        zp, pst = ctx.bgzf_compress(part)
        nb = stats["blocks"] - 1
        return {"what": what, "reads": a.reads, "sam_bytes": n, "bytes_per_read": n / a.reads, "aligned": ast["aligned"], "align_step_ms": align_ms,
                "pinned_text": t_pinned, "pageable_text": t_pageable, "ms_per_million_reads_kernel": t_pinned["t_kernel_ms"]["median"] * 1e6 / a.reads,
                "ms_per_million_reads_total": t_pinned["t_total_ms"]["median"] * 1e6 / a.reads, **stats,
                "matches_per_block": stats["matches"] / nb, "literals_per_block": stats["literals"] / nb, "ratio": stats["out_bytes"] / n,
                "zlib_sample_bytes": len(part), "ratio_on_sample": len(zp) / len(part), "zlib1_ratio_on_sample": z1_n / len(part),
                "zlib6_ratio_on_sample": z6_n / len(part), "zlib1_one_core_MB_per_s": len(part) / z1_s / 1e6,
                "zlib1_sixteen_cores_ms_for_the_text": n / (16 * len(part) / z1_s) * 1e3, "zlib6_one_core_MB_per_s": len(part) / z6_s / 1e6}

    out = {"steps": a.steps, "warmup": a.warmup, "block_size": BS,
           "constant_qualities": leg(np.full(reads.size, ord("I"), dtype=np.uint8), "qualities all 'I' (the benchmark's reads)"),
           "binned_phred_qualities": leg(realistic_quals(a.reads, a.read_len, 7), "qualities from a binned Phred distribution")}
    print(json.dumps(out))
    ctx.close()
    idx.close()


if __name__ == "__main__":
    main()
