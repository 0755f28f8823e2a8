"""sc_plan / sc_segment / sc_seg_count / sc_task_of (moni_align_amd/csrc/seqcount_core.h: what seqcount_plan_kernel and seqcount_walk_kernel run per
lane) replayed on the host over the device index image, against the plain-Python model of tests/seqcount_model.py: every field of every record,
every entry of the table and the phi-step count, no tolerance.  The same replay runs once more as a stand-alone program under the address and
undefined-behaviour sanitizers.  The real kernels are checked against brute force under -m gpu."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from moni_align_amd import capi
from tests import locate_model as lm
from tests import seqcount_model as sm
from tests.test_host_sim import long_run_case

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sim")
SRC = os.path.join(HERE, "seqcount_sim.cpp")
DEPS = [SRC] + [os.path.join(capi.CSRC, f) for f in ("seqcount_core.h", "locate_core.h", "seed_core.h", "image.hpp", "layout.h")] + \
       [os.path.join(os.path.dirname(capi.HERE), "include", "moni_hip.h")]
_lib = None


def stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS)


def sim_lib():
    """tests/host_sim/libseqcount_sim.so, built beside the other host-sim libraries and leaving them alone"""
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "libseqcount_sim.so")
        if stale(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", so, SRC])
        L = C.CDLL(so)
        L.scsim_create.restype = C.c_void_p
        L.scsim_create.argtypes = [C.POINTER(capi.FlatIndexC)]
        L.scsim_destroy.argtypes = [C.c_void_p]
        L.scsim_n_seq.restype = C.c_uint32
        L.scsim_n_seq.argtypes = [C.c_void_p]
        L.scsim_run.restype = C.c_uint64
        L.scsim_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


class ScSim:
    def __init__(self, fi, without_lcp=False):
        self.fi = fi
        st = capi.flat_struct(fi, without_lcp=without_lcp)
        self.h = sim_lib().scsim_create(C.byref(st))
        if not self.h:
            raise RuntimeError("seqcount_sim: index rejected")

    def run(self, patterns, strands=1, max_walk=1 << 20):
        seq, offs = lm.ragged(patterns)
        n = len(patterns)
        n_seq = sim_lib().scsim_n_seq(self.h)
        res = np.zeros(n * strands + 1, dtype=sm.RES_DTYPE)
        counts = np.zeros((n * strands + 1, n_seq), dtype=np.uint64)
        cnt = np.zeros(4, dtype=np.uint64)
        seq = np.concatenate([seq, np.zeros(8, np.uint8)])
        segs = sim_lib().scsim_run(self.h, seq.ctypes.data, offs.ctypes.data, n, strands, max_walk, res.ctypes.data, counts.ctypes.data, cnt.ctypes.data)
        return res[:-1], counts[:-1], cnt, segs

    def close(self):
        if self.h:
            sim_lib().scsim_destroy(self.h)
            self.h = None


def compare(got_res, got_counts, got_phi, got_segs, want):
    for k in sm.RES_DTYPE.names:
        assert np.array_equal(got_res[k], want[0][k]), (k, np.nonzero(got_res[k] != want[0][k])[0][:5])
    assert np.array_equal(got_counts, want[1])
    assert got_phi == want[2] and got_segs == int(want[0]["n_segs"].sum())
    w = want[0]["walked"] != 0
    assert want[2] == int((want[0]["count"][w].astype(np.int64) - want[0]["n_segs"][w]).sum())


def check(fi, patterns, strands, max_walk, without_lcp=False):
    sim = ScSim(fi, without_lcp)
    try:
        want = sm.SeqcountModel(fi).seq_batch(patterns, strands, max_walk)
        res, counts, cnt, segs = sim.run(patterns, strands, max_walk)
        compare(res, counts, int(cnt[2]), int(segs), want)
        return res, counts, cnt
    finally:
        sim.close()


def segment_shapes(fi, patterns, res, strands):
    """which of the shapes a segment walk can go wrong at this batch holds"""
    model = sm.SeqcountModel(fi)
    have = set()
    for t, r in enumerate(res):
        if not int(r["walked"]):
            have.add("over max_walk")
            continue
        if int(r["count"]) == 1:
            have.add("count 1")
        if int(r["n_segs"]) == 1:
            have.add("one segment")
        if int(r["n_segs"]) >= 3:
            have.add("three segments")
        if int(r["n_segs"]) >= 100:
            have.add("hundreds of segments")
        if int(r["n_segs"]) >= 1:
            p = patterns[t // strands]
            count, sa_lo, matched, toe = model.search(lm.revcomp(p) if t % strands else p)
            segs = model.segments(sa_lo, count, toe)
            if segs[-1][1] == 1:
                have.add("last segment of length 1")
            if max(ln for _, ln in segs) >= 4096:
                have.add("segment past the 12-bit length")
            heads = set(model.heads[k] for k in range(model.run_of_position(sa_lo), model.run_of_position(sa_lo + count - 1)))
            if ord("N") in heads:
                have.add("head rank from cr")
    return have


@pytest.mark.parametrize("strands,max_walk", [(1, 1 << 20), (2, 0), (2, 8)])
def test_planted_case(strands, max_walk):
    fi, text, pats = lm.planted_case()
    pats = pats + [b"A", b"C", b"G", b"T", b"AC"]
    res, counts, cnt = check(fi, pats, strands, max_walk)
    sm.check_against_brute(text, pats, res, counts, strands, max_walk, fi.seq_starts)
    have = segment_shapes(fi, pats, res, strands)
    want = {"count 1", "one segment", "three segments", "last segment of length 1"}
    want |= {"over max_walk"} if max_walk == 8 else {"hundreds of segments", "head rank from cr"}
    assert want <= have, want - have
    unit = res[19 * strands]
    assert int(unit["count"]) >= 9 and int(unit["walked"]) == (0 if max_walk == 8 else 1)
    assert int(cnt[3]) > 0                                       # N has no hot slot: the search took the general path


def test_without_lcp_samples():
    fi, text, pats = lm.planted_case()
    res, counts, cnt = check(fi, pats, 2, 1 << 20, without_lcp=True)
    sm.check_against_brute(text, pats, res, counts, 2, 1 << 20, fi.seq_starts)


def test_long_runs_and_cold_letters():
    """W occurs 6000 times behind one BWT run of 4095 or more (a segment longer than the 12-bit length field, a row that is not "ok"); a one-letter
    pattern whose interval spans hundreds of runs, some of them runs of N (the head rank comes from cr)"""
    fi, reads = long_run_case()
    reads = [r.tobytes() for r in reads]
    text = fi.text.tobytes()
    W = text[13:53]
    pats = [W, W[:20], W[5:], b"C" + W, text[12:53], b"A", b"N", b"NNNN", b"ANNNN"] + [r[100:130] for r in reads[:40]] + [text[a:a + 60] for a in range(0, 60000, 6000)]
    assert len(lm.occurrences(text, W)) == 6000
    res, counts, cnt = check(fi, pats, 2, 1 << 20)
    assert int(res["count"][0]) == 6000 and int(counts[0, 0]) == 6000 and int(res["n_seqs"][0]) == 1
    have = segment_shapes(fi, pats, res, 2)
    want = {"count 1", "one segment", "three segments", "hundreds of segments", "segment past the 12-bit length", "head rank from cr"}
    assert want <= have, want - have
    lens = np.diff(fi.starts.astype(np.int64))
    k = int(np.searchsorted(fi.starts.astype(np.int64), int(res["sa_lo"][0]), side="right")) - 1          # W's interval lies inside one run that is not "ok"
    assert int(lens[k]) >= 4095 and int(res["n_segs"][0]) == 1
    check(fi, pats[:12], 1, 8)                                   # the limit: W and its substrings are counted, not enumerated


def test_standalone_program_under_sanitizers(tmp_path):
    """the same per-lane code in a program of its own, compiled with -fsanitize=address,undefined and run as a child process on the planted case:
    it must end clean and give the model's values (the sanitizers' runtimes are linked statically: the program needs nothing from its environment)"""
    exe = os.path.join(HERE, "seqcount_sim_asan")
    if stale(exe):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                               "-DSEQCOUNT_SIM_MAIN", "-o", exe, SRC])
    fi, text, pats = lm.planted_case()
    pats = pats + [b"A"]
    for strands, max_walk, with_lcp in ((2, 1 << 20, 1), (1, 8, 0)):
        seq, offs = lm.ragged(pats)
        n_seq = len(fi.seq_starts) - 1
        u64 = lambda a: np.ascontiguousarray(a, dtype=np.uint64).tobytes()
        blob = u64([fi.n, fi.r, fi.w, n_seq, with_lcp, len(pats), strands, max_walk]) + u64(fi.F) + u64(fi.starts) + u64(fi.ssa) + u64(fi.esa) + u64(fi.thr)
        blob += (u64(fi.slcp) if with_lcp else b"") + u64(fi.seq_starts) + u64(offs) + np.ascontiguousarray(fi.heads, dtype=np.uint8).tobytes() + seq.tobytes()
        src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
        src.write_bytes(blob)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([exe, str(src), str(dst)], env=env, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-2000:]
        raw = dst.read_bytes()
        nt = len(pats) * strands
        assert len(raw) == nt * 32 + nt * n_seq * 8 + 40
        res = np.frombuffer(raw[:nt * 32], dtype=sm.RES_DTYPE)
        counts = np.frombuffer(raw[nt * 32:nt * 32 + nt * n_seq * 8], dtype=np.uint64).reshape(nt, n_seq)
        tail = np.frombuffer(raw[-40:], dtype=np.uint64)
        compare(res, counts, int(tail[2]), int(tail[4]), sm.SeqcountModel(fi).seq_batch(pats, strands, max_walk))
