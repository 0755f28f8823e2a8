"""loci_key / loci_seg_hi / loci_seg_keys / loci_is_head (moni_align_amd/csrc/loci_core.h: what loci_walk_kernel and the fold kernels run per lane)
replayed on the host over the device index image and the lift tables, against the plain-Python model of tests/loci_model.py: every field of every
record, the four arrays, the phi-step count and the segments, no tolerance.  The same replay runs once more as a stand-alone program under the
address and undefined-behaviour sanitizers, its key buffer sized to the walked total exactly.  The real kernels are checked against brute force
under -m gpu."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from moni_align_amd import capi
from tests import locate_model as lm
from tests import loci_model as lo
from tests.test_host_sim import long_run_case

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sim")
SRC = os.path.join(HERE, "loci_sim.cpp")
DEPS = [SRC] + [os.path.join(capi.CSRC, f) for f in ("loci_core.h", "lift_core.h", "lift_build.hpp", "seqcount_core.h", "locate_core.h", "seed_core.h", "image.hpp", "layout.h")] + \
       [os.path.join(os.path.dirname(capi.HERE), "include", "moni_hip.h")]
_lib = None


def stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS)


def sim_lib():
    """tests/host_sim/libloci_sim.so, built beside the other host-sim libraries and leaving them alone"""
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "libloci_sim.so")
        if stale(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", so, SRC])
        L = C.CDLL(so)
        L.locisim_create.restype = C.c_void_p
        L.locisim_create.argtypes = [C.POINTER(capi.FlatIndexC)]
        L.locisim_destroy.argtypes = [C.c_void_p]
        L.locisim_run.restype = None
        L.locisim_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.locisim_fetch.restype = None
        L.locisim_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.locisim_key.restype = C.c_uint64
        L.locisim_key.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32]
        L.locisim_key_shape.restype = C.c_uint32
        L.locisim_key_shape.argtypes = [C.c_void_p, C.c_uint64]
        _lib = L
    return _lib


class LociSim:
    def __init__(self, fi, without_lcp=False):
        self.fi = fi
        st = capi.flat_struct(fi, without_lcp=without_lcp)
        self.h = sim_lib().locisim_create(C.byref(st))
        if not self.h:
            raise RuntimeError("loci_sim: index rejected")

    def run(self, patterns, strands=1, lift=1, max_walk=1 << 20):
        """((res, lpos, lseq, lseq_off, support), counters, segments, walked total)"""
        seq, offs = lm.ragged(patterns)
        n = len(patterns)
        res = np.zeros(n * strands + 1, dtype=lo.RES_DTYPE)
        sizes, cnt = np.zeros(3, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        seq = np.concatenate([seq, np.zeros(8, np.uint8)])
        sim_lib().locisim_run(self.h, seq.ctypes.data, offs.ctypes.data, n, strands, lift, max_walk, res.ctypes.data, sizes.ctypes.data, cnt.ctypes.data)
        k = int(sizes[0])
        lp, ls, lso, su = np.zeros(k + 1, np.uint64), np.zeros(k + 1, np.uint32), np.zeros(k + 1, np.uint64), np.zeros(k + 1, np.uint64)
        sim_lib().locisim_fetch(lp.ctypes.data, ls.ctypes.data, lso.ctypes.data, su.ctypes.data)
        return (res[:-1], lp[:k], ls[:k], lso[:k], su[:k]), cnt, int(sizes[1]), int(sizes[2])

    def key(self, pos, lift=1):
        return int(sim_lib().locisim_key(self.h, pos, lift))

    def shape(self, pos):
        return int(sim_lib().locisim_key_shape(self.h, pos))

    def close(self):
        if self.h:
            sim_lib().locisim_destroy(self.h)
            self.h = None


def compare(got, got_phi, got_segs, got_total, want):
    for k in lo.RES_DTYPE.names:
        assert np.array_equal(got[0][k], want[0][k]), (k, np.nonzero(got[0][k] != want[0][k])[0][:5])
    for a, b, name in zip(got[1:5], want[1:5], ("lpos", "lseq", "lseq_off", "support")):
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    w = want[0]["walked"] != 0
    assert got_phi == want[5] == int((want[0]["count"][w].astype(np.int64) - want[0]["n_segs"][w]).sum())
    assert got_segs == int(want[0]["n_segs"].sum()) and got_total == int(want[0]["count"][w].sum()) == int(want[4].sum())


def check(fi, patterns, strands, lift, max_walk, without_lcp=False):
    sim = LociSim(fi, without_lcp)
    try:
        want = lo.LociModel(fi).loci_batch(patterns, strands, lift, max_walk)
        got, cnt, segs, total = sim.run(patterns, strands, lift, max_walk)
        compare(got, int(cnt[2]), segs, total, want)
        return got, cnt
    finally:
        sim.close()


SHAPES = {1: "sequence moved past the directory's", 2: "hint run walked forward", 4: "last directory block", 8: "inside an insertion", 16: "just behind a deletion"}


def shapes_held(fi, text, patterns, res, strands):
    """which of the shapes the walk and the lift can go wrong at this batch holds; every occurrence's key is checked against the model on the way"""
    have = set()
    sim, model = LociSim(fi), lo.LociModel(fi)
    try:
        for t, r in enumerate(res):
            if not int(r["walked"]):
                have.add("over max_walk")
                continue
            if int(r["n_segs"]) == 1:
                have.add("one segment")
            if int(r["n_segs"]) >= 200:
                have.add("hundreds of segments")
            p = patterns[t // strands]
            if not p:
                have.add("empty pattern")
            for pos in lm.occurrences(text, lm.revcomp(p) if t % strands else p):
                assert sim.key(pos) == model.lift(pos) and sim.key(pos, 0) == pos
                s = sim.shape(pos)
                have |= {name for bit, name in SHAPES.items() if s & bit}
    finally:
        sim.close()
    return have


@pytest.mark.parametrize("strands,lift,max_walk", [(1, 1, 1 << 20), (2, 1, 0), (2, 0, 1 << 20), (2, 1, 8)])
def test_lifted_case(strands, lift, max_walk):
    pg, fi, text, pats = lo.lifted_case()
    got, cnt = check(fi, pats, strands, lift, max_walk)
    lo.check_against_brute(text, pats, got, strands, max_walk, fi.seq_starts, lo.text_to_ref(pg) if lift else None)
    have = shapes_held(fi, text, pats, got[0], strands)
    want = {"one segment", "empty pattern", "hint run walked forward", "last directory block", "inside an insertion", "just behind a deletion"}
    want |= {"over max_walk"} if max_walk == 8 else {"hundreds of segments"}
    assert want <= have, want - have
    if lift and max_walk != 8:
        assert int(got[4].max()) > len(pg.seqs)                 # a locus with more support than there are sequences: an insertion folded
        a = int(got[0]["loci_off"][2 * strands])
        assert int(got[0]["n_loci"][2 * strands]) == 1 and (int(got[1][a]), int(got[4][a])) == (1000, len(pg.seqs))          # the reference 32-mer: one locus, every sequence
    if not lift:
        assert (got[4] == 1).all()


def test_null_lifts():
    """the FASTA-built form of the same text: lift = 1 equals lift = 0"""
    pg, fi, text, pats = lo.lifted_case(lifted=False)
    a, _ = check(fi, pats, 2, 1, 1 << 20)
    b, _ = check(fi, pats, 2, 0, 1 << 20)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    lo.check_against_brute(text, pats, a, 2, 1 << 20, fi.seq_starts, None)


@pytest.mark.parametrize("strands,lift,max_walk,without_lcp", [(2, 1, 1 << 20, False), (1, 0, 8, False), (2, 0, 0, True)])
def test_planted_case(strands, lift, max_walk, without_lcp):
    """three unrelated sequences, null lifts: N runs (the general path of the search), separators and terminator bytes in patterns"""
    fi, text, pats = lm.planted_case()
    pats = pats + [b"A", b"C", b"AC"]
    got, cnt = check(fi, pats, strands, lift, max_walk, without_lcp)
    assert int(cnt[3]) > 0 and (got[4] == 1).all()
    unit = got[0][19 * strands]
    assert int(unit["count"]) >= 9 and int(unit["walked"]) == (0 if max_walk == 8 else 1) and int(unit["n_loci"]) == (0 if max_walk == 8 else int(unit["count"]))


def test_long_runs_and_cold_letters():
    """W occurs 6000 times behind one BWT run of 4095 or more (one segment of 6000 slots, filled from the top); a one-letter pattern whose interval
    spans hundreds of runs"""
    fi, reads = long_run_case()
    text = fi.text.tobytes()
    W = text[13:53]
    pats = [W, W[:20], b"C" + W, b"A", b"N", b"NNNN"] + [text[a:a + 60] for a in range(0, 60000, 6000)]
    got, cnt = check(fi, pats, 2, 1, 1 << 20)
    assert int(got[0]["count"][0]) == 6000 and int(got[0]["n_segs"][0]) == 1 and int(got[0]["n_loci"][0]) == 6000
    assert int(got[0]["n_segs"].max()) >= 200
    check(fi, pats[:6], 1, 0, 8)


def test_standalone_program_under_sanitizers(tmp_path):
    """the same per-lane code in a program of its own, compiled with -fsanitize=address,undefined and run as a child process on the lifted case:
    it must end clean and give the model's values (the sanitizers' runtimes are linked statically: the program needs nothing from its environment)"""
    exe = os.path.join(HERE, "loci_sim_asan")
    if stale(exe):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                               "-DLOCI_SIM_MAIN", "-o", exe, SRC])
    pg, fi, text, pats = lo.lifted_case()
    lf = fi.lifts
    for strands, lift, max_walk, with_lcp in ((2, 1, 1 << 20, 1), (1, 1, 8, 0), (2, 0, 0, 1)):
        seq, offs = lm.ragged(pats)
        n_seq = len(fi.seq_starts) - 1
        u64 = lambda a: np.ascontiguousarray(a, dtype=np.uint64).tobytes()
        blob = u64([fi.n, fi.r, fi.w, n_seq, with_lcp, len(pats), strands, max_walk, lift, 1]) + u64(fi.F) + u64(fi.starts) + u64(fi.ssa) + u64(fi.esa) + u64(fi.thr)
        blob += (u64(fi.slcp) if with_lcp else b"") + u64(fi.seq_starts) + u64(offs)
        blob += u64(lf.second) + u64(lf.len) + u64(lf.ins_off) + u64(lf.ins) + u64(lf.del_off) + u64(lf.dele)
        blob += np.ascontiguousarray(fi.heads, dtype=np.uint8).tobytes() + seq.tobytes()
        src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
        src.write_bytes(blob)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([exe, str(src), str(dst)], env=env, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and "ERROR" not in p.stderr and "runtime error" not in p.stderr and "loci_sim:" not in p.stderr, p.stderr[-2000:]
        raw = dst.read_bytes()
        nt = len(pats) * strands
        tail = np.frombuffer(raw[-56:], dtype=np.uint64)
        k = int(tail[6])
        assert len(raw) == nt * 48 + 4 * k * 8 + 56
        res = np.frombuffer(raw[:nt * 48], dtype=lo.RES_DTYPE)
        arr = np.frombuffer(raw[nt * 48:nt * 48 + 4 * k * 8], dtype=np.uint64).reshape(4, k)
        got = (res, arr[0], arr[3].astype(np.uint32), arr[1], arr[2])
        compare(got, int(tail[2]), int(tail[4]), int(tail[5]), lo.LociModel(fi).loci_batch(pats, strands, lift, max_walk))
