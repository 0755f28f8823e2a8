"""Rate of the BGZF reader (moni_bgzf_inflate) on the benchmark's workload: the FASTQ text of the 1 M x 150 bp reads, with constant and with binned-Phred
qualities, compressed with zlib level 6 into 65280-byte BGZF members (on the host, sixteen processes); one context, 3 warm-up + 10 timed calls;
median (min - max) of the library's own figures - t_kernel (HIP events around the kernel) and t_total (with the upload of the members and the
download of the text).  Yardsticks from the same process: zlib.decompress over the same members on one host core, and the align step
(moni_align_stream, one context) on the same reads.  Prints one JSON line.

    python profiles/inflate_rate.py [--cache DIR] [--base-len N --haps H] [--reads N] [--steps K] [--warmup W] [--zlib-mb M]

The index file must exist (a bench.py run with the same --base-len / --haps writes it); nothing is built here."""
import argparse
import ctypes as C
import json
import multiprocessing
import os
import struct
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from profiles.bgzf_rate import realistic_quals, spread          # noqa: E402

BS = 65280
HEADER = bytes.fromhex("1f8b08040000000000ff060042430200")


def member(block: bytes) -> bytes:
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    z = c.compress(block) + c.flush()
    return HEADER + struct.pack("<H", 18 + len(z) + 8 - 1) + z + struct.pack("<II", zlib.crc32(block) & 0xFFFFFFFF, len(block))


def fastq_text(reads: np.ndarray, quals: np.ndarray) -> bytes:
    n, L = reads.shape
    parts, lo = [], 0
    while lo < n:          # records in blocks of equal name length
        digits = len(str(lo))
        hi = min(n, 10 ** digits)
        name = np.frombuffer(("@simulated." + "0" * digits + "\n").encode(), np.uint8)
        rec = np.empty((hi - lo, len(name) + L + 1 + 2 + L + 1), np.uint8)
        rec[:, :len(name)] = name
        idx = np.arange(lo, hi)
        for d in range(digits):
            rec[:, len(name) - 2 - d] = (idx // 10 ** d) % 10 + 48
        o = len(name)
        rec[:, o:o + L] = reads[lo:hi]; rec[:, o + L] = 10
        rec[:, o + L + 1] = ord("+"); rec[:, o + L + 2] = 10
        rec[:, o + L + 3:o + 2 * L + 3] = quals[lo:hi]; rec[:, o + 2 * L + 3] = 10
        parts.append(rec.tobytes())
        lo = hi
    return b"".join(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache", default="/tmp/moni_bench_cache")
    ap.add_argument("--base-len", type=int, default=61420004)
    ap.add_argument("--haps", type=int, default=12)
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--zlib-mb", type=int, default=64, help="megabytes of the text the host's zlib.decompress leg takes")
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
    idx = capi.Index(path=path, device=0)
    ctx = capi.Ctx(idx)
    L = capi.lib()

    def align_ms(quals):
        for _ in range(2):
            ctx.align_batch(reads.reshape(-1), offs, names, noff, quals, stream=True, want_text=False)
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            ctx.align_batch(reads.reshape(-1), offs, names, noff, quals, stream=True, want_text=False)
            t.append(time.perf_counter() - t0)
        return spread(t, 1e3)

    def leg(quals, what):
        text = fastq_text(reads, quals.reshape(a.reads, a.read_len))
        with multiprocessing.Pool(16) as pool:
            members = pool.map(member, [text[at:at + BS] for at in range(0, len(text), BS)], chunksize=64)
        z = b"".join(members)
        buf = np.frombuffer(z, dtype=np.uint8)
        p = capi.InflateParamsC()
        L.moni_inflate_params_default(C.byref(p))
        out, on, st = C.c_void_p(), C.c_uint64(), capi.InflateStatsC()
        tk, tt = [], []
        for k in range(a.warmup + a.steps):
            rc = L.moni_bgzf_inflate(ctx._h, buf.ctypes.data, buf.size, C.byref(p), C.byref(out), C.byref(on), C.byref(st))
            if rc:
                sys.exit("moni_bgzf_inflate failed with code %d (member %d, reason %d)" % (rc, st.first_bad_block, st.bad_reason))
            if k >= a.warmup:
                tk.append(st.t_kernel); tt.append(st.t_total)
        assert C.string_at(out.value, on.value) == text
        stats = {k: getattr(st, k) for k, _ in capi.InflateStatsC._fields_ if not k.startswith("t_") and k != "pad"}
        nz = max(1, min(len(members), (a.zlib_mb << 20) // BS))
        t0 = time.perf_counter()
        got = sum(len(zlib.decompress(m[18:-8], -15)) for m in members[:nz])
        zs = time.perf_counter() - t0
        n = len(text)
        return {"what": what, "reads": a.reads, "text_bytes": n, "compressed_bytes": len(z), "ratio": len(z) / n, **stats,
                "t_kernel_ms": spread(tk, 1e3), "t_total_ms": spread(tt, 1e3), "transfers_ms": spread([x - y for x, y in zip(tt, tk)], 1e3),
                "kernel_GB_per_s_of_text": n / float(np.median(tk)) / 1e9, "total_GB_per_s_of_text": n / float(np.median(tt)) / 1e9,
                "Mreads_per_s_total": a.reads / float(np.median(tt)) / 1e6,
                "zlib_decompress_sample_bytes": got, "zlib_decompress_one_core_MB_per_s": got / zs / 1e6,
                "zlib_decompress_one_core_ms_for_the_text": n / (got / zs) * 1e3, "align_step_ms": align_ms(quals)}

    out = {"steps": a.steps, "warmup": a.warmup, "block_size": BS, "zlib_level": 6,
           "constant_qualities": leg(np.full(reads.size, ord("I"), dtype=np.uint8), "qualities all 'I' (the benchmark's reads)"),
           "binned_phred_qualities": leg(realistic_quals(a.reads, a.read_len, 7), "qualities from a binned Phred distribution")}
    print(json.dumps(out))
    ctx.close()
    idx.close()


if __name__ == "__main__":
    main()
