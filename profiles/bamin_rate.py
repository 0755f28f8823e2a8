"""Rate of the BAM reader (moni_bam_in_feed) on the benchmark's workload: the 1 M x 150 bp reads as unaligned BAM, zlib level 6,
65280-byte members (made on the host, sixteen processes); one context, 3 warm-up + 10 timed feeds of the whole file (a reset before each); median
(min - max) of every phase of t_kernel and of t_total.  Beside it, from the same process and the same members: moni_bgzf_inflate, what the parent
could already do to this file - so the table says what the record layer costs on top of inflation and which phase takes it.  Prints one JSON line.

    python profiles/bamin_rate.py [--cache DIR] [--base-len N --haps H] [--reads N] [--steps K] [--warmup W]

The index file must exist (a bench.py run with the same --base-len / --haps writes it); nothing is built here.

    python profiles/bamin_rate.py --frontend
takes profiles/frontend.py's reads (/tmp/frontend_reads.fq), makes the bgzipped FASTQ and the unaligned BAM of them, and runs moni-hip-align on
each, twice in turn (profiles/frontend_bgzf.py's procedure): steady-state reads/s, the reader thread's three counters, the outputs compared."""
import argparse
import ctypes as C
import json
import multiprocessing
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from profiles.bgzf_rate import spread          # noqa: E402
from profiles.inflate_rate import BS, member          # noqa: E402

EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BAM_HEADER = b"BAM\x01" + (24).to_bytes(4, "little") + b"@HD\tVN:1.6\tSO:unsorted\n\x00"[:24] + (0).to_bytes(4, "little")
CODE = np.full(256, 15, np.uint8)
for _k, _c in enumerate(b"=ACMGRSVTWYHKDBN"):
    CODE[_c] = _k


def ubam_records(reads: np.ndarray, quals: np.ndarray, first: int = 0) -> bytes:
    """unaligned records (flag 4) named simulated.<first + i>, in blocks of equal name length; quals: ASCII"""
    n, L = reads.shape
    assert L % 2 == 0
    codes = CODE[reads]
    packed = (codes[:, 0::2] << 4 | codes[:, 1::2]).astype(np.uint8)
    parts, lo = [], 0
    while lo < n:
        digits = len(str(first + lo))
        hi = min(n, 10 ** digits - first)
        name = np.frombuffer(("simulated." + "0" * digits + "\0").encode(), np.uint8)
        size = 32 + len(name) + L // 2 + L
        fixed = np.frombuffer(np.array([size, -1, -1], "<i4").tobytes() + bytes([len(name), 0]) + np.array([4680, 0, 4], "<u2").tobytes() + np.array([L, -1, -1, 0], "<i4").tobytes(), np.uint8)
        rec = np.empty((hi - lo, 4 + size), np.uint8)
        rec[:, :36] = fixed
        rec[:, 36:36 + len(name)] = name
        idx = np.arange(first + lo, first + hi)
        for d in range(digits):
            rec[:, 36 + len(name) - 2 - d] = (idx // 10 ** d) % 10 + 48
        o = 36 + len(name)
        rec[:, o:o + L // 2] = packed[lo:hi]
        rec[:, o + L // 2:] = quals[lo:hi] - 33
        parts.append(rec.tobytes())
        lo = hi
    return b"".join(parts)


def bgzip16(data, pool) -> bytes:
    return b"".join(pool.map(member, [bytes(data[at:at + BS]) for at in range(0, len(data), BS)], chunksize=64)) + EOF_MEMBER


def rate(a):
    from moni_align_amd import capi, synth
    from profiles.inflate_rate import fastq_text
    path = os.path.join(a.cache, "idx_%d_%d_lifted_0.mfi" % (a.base_len, a.haps))
    if not os.path.exists(path):
        sys.exit("no cached index %s: run bench.py with the same --base-len / --haps first" % path)
    pg = synth.make_pangenome(a.base_len, a.haps, seed=19, var_seed=12)
    reads = synth.make_reads(pg, a.reads, a.read_len, seed=150)
    del pg
    quals = np.full(reads.shape, ord("I"), np.uint8)
    raw = BAM_HEADER + ubam_records(reads, quals)
    with multiprocessing.Pool(16) as pool:
        z = bgzip16(raw, pool)
    idx = capi.Index(path=path, device=0)
    ctx = capi.Ctx(idx)
    L = capi.lib()
    buf = np.frombuffer(z, dtype=np.uint8)
    phases = {k: [] for k in capi.BAMIN_PHASES}
    tt = []
    for k in range(a.warmup + a.steps):
        ctx.bam_in_reset()
        t1, _, n, st = ctx.bam_in_feed(buf, last=True)
        if k >= a.warmup:
            for p, v in st["t_kernel"].items():
                phases[p].append(v)
            tt.append(st["t_total"])
    assert n == a.reads and t1 == fastq_text(reads, quals), "the text is not the reads' FASTQ"
    ip = capi.InflateParamsC()
    L.moni_inflate_params_default(C.byref(ip))
    out, on, ist = C.c_void_p(), C.c_uint64(), capi.InflateStatsC()
    ik, it = [], []
    for k in range(a.warmup + a.steps):
        assert L.moni_bgzf_inflate(ctx._h, buf.ctypes.data, buf.size, C.byref(ip), C.byref(out), C.byref(on), C.byref(ist)) == 0
        if k >= a.warmup:
            ik.append(ist.t_kernel); it.append(ist.t_total)
    assert on.value == len(raw)
    res = {"steps": a.steps, "warmup": a.warmup, "block_size": BS, "zlib_level": 6, "reads": a.reads, "bam_bytes": len(raw), "compressed_bytes": len(z), "text_bytes": len(t1),
           "records": st["records"], "members": st["inflate"]["blocks"],
           "bam_in_feed_ms": {"t_kernel": {p: spread(v, 1e3) for p, v in phases.items()}, "t_total": spread(tt, 1e3)},
           "bgzf_inflate_same_members_ms": {"t_kernel": spread(ik, 1e3), "t_total": spread(it, 1e3)},
           "record_layer_kernels_ms_median": sum(float(np.median(phases[p])) for p in ("find", "select", "text")) * 1e3,
           "Mreads_per_s_total": a.reads / float(np.median(tt)) / 1e6}
    print(json.dumps(res))
    ctx.close()
    idx.close()


def frontend(a):
    fq, fz, fb = "/tmp/frontend_reads.fq", "/tmp/frontend_reads.fq.gz", "/tmp/frontend_reads.bam"
    mfi = os.path.join(a.cache, "idx_%d_%d_lifted_0" % (a.base_len, a.haps))
    exe = os.path.join(ROOT, "moni_align_amd", "host", "moni-hip-align")
    L, t0 = a.read_len, time.time()
    text = np.memmap(fq, dtype=np.uint8, mode="r")
    with multiprocessing.Pool(16) as pool, open(fz, "wb") as g, open(fb, "wb") as h:
        at, lo, first = 0, 0, True
        while at < len(text):          # records in blocks of equal name length, as profiles/frontend.py writes them
            digits = len(str(lo))
            width = len("@simulated.\n") + digits + 2 * L + 4
            k = min(10 ** digits - lo, (len(text) - at) // width, 2000000)
            blk = np.asarray(text[at:at + k * width]).reshape(k, width)
            o = len("@simulated.\n") + digits
            assert bytes(blk[0, :o]) == b"@simulated.%d\n" % lo
            g.write(bgzip16(blk.reshape(-1), pool)[:-len(EOF_MEMBER)])
            h.write(bgzip16((BAM_HEADER if first else b"") + ubam_records(blk[:, o:o + L], blk[:, o + L + 3:o + 2 * L + 3], lo), pool)[:-len(EOF_MEMBER)])
            at, lo, first = at + k * width, lo + k, False
        g.write(EOF_MEMBER); h.write(EOF_MEMBER)
    print("%d reads: bgzipped FASTQ %.2f GB, unaligned BAM %.2f GB, made in %.0fs" % (lo, os.path.getsize(fz) / 1e9, os.path.getsize(fb) / 1e9, time.time() - t0), flush=True)

    def run(inp, out):
        cmd = [exe, mfi, "-p", inp, "-o", out, "-t", "16", "-S", "1000", "-F", "0.5"]
        t = time.time()
        r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, MONI_CLI_VERBOSE="1"), timeout=300)
        wall = time.time() - t
        if r.returncode:
            print(r.stderr[-3000:]); sys.exit("CLI failed with %d" % r.returncode)
        rng = sorted((int(m.group(1)), int(m.group(2)), float(m.group(3))) for m in re.finditer(r"range (\d+) \(worker \d+, (\d+) reads\).*done at ([0-9.]+) s", r.stderr))
        n = len(rng)
        k0, k1 = (3 * n + 7) // 8, n - 2
        reads = sum(x[1] for x in rng[k0:k1 + 1])
        dt = rng[k1][2] - rng[k0 - 1][2]
        tail = [l for l in r.stderr.splitlines() if "Reads per second" in l or "Stage seconds" in l or " input " in l or "Elapsed" in l]
        res = {"input": inp, "wall_s": wall, "ranges": n, "steady_ranges": [k0, k1], "steady_reads": reads, "steady_s": dt, "steady_Mreads_per_s": reads / dt / 1e6,
               "done_at_s": [x[2] for x in rng], "lines": tail}
        print(json.dumps(res), flush=True)
        return res

    res = {"bgzf": run(fz, "/tmp/fe_bgzf.sam"), "bam": run(fb, "/tmp/fe_bam.sam"), "bgzf_again": run(fz, "/tmp/fe_bgzf2.sam"), "bam_again": run(fb, "/tmp/fe_bam2.sam")}
    res["outputs_identical"] = subprocess.run(["cmp", "/tmp/fe_bgzf.sam", "/tmp/fe_bam.sam"]).returncode == 0
    res["ratio"] = res["bam"]["steady_Mreads_per_s"] / res["bgzf"]["steady_Mreads_per_s"]
    res["ratio_again"] = res["bam_again"]["steady_Mreads_per_s"] / res["bgzf_again"]["steady_Mreads_per_s"]
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache", default="/tmp/moni_bench_cache")
    ap.add_argument("--base-len", type=int, default=61420004)
    ap.add_argument("--haps", type=int, default=12)
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frontend", action="store_true")
    args = ap.parse_args()
    (frontend if args.frontend else rate)(args)
