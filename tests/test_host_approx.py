"""apx_exact / apx_piece / apx_task_of (moni_align_amd/csrc/approx_core.h: what approx_exact_kernel and approx_tree_kernel run per lane) and
loc_walk replayed on the host over the device index image, the passes in launch order, against the plain-Python model of tests/approx_model.py:
every field of every record, the sorted hits, every position, the tree steps and the phi steps, no tolerance.  The inputs are asserted to hold
the shapes the walk can go wrong at.  The same replay runs once more as a stand-alone program under the address and undefined-behaviour
sanitizers.  The real kernels are checked against brute force under -m gpu."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from moni_align_amd import capi
from tests import approx_model as am
from tests import locate_model as lm

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sim")
SRC = os.path.join(HERE, "approx_sim.cpp")
DEPS = [SRC] + [os.path.join(capi.CSRC, f) for f in ("approx_core.h", "locate_core.h", "seed_core.h", "image.hpp", "layout.h")] + \
       [os.path.join(os.path.dirname(capi.HERE), "include", "moni_hip.h")]
DEFAULT = am.MAX_STEPS_DEFAULT
_lib = None


def stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS)


def sim_lib():
    """tests/host_sim/libapprox_sim.so, built beside the other host-sim libraries and leaving them alone"""
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "libapprox_sim.so")
        if stale(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", so, SRC])
        L = C.CDLL(so)
        L.apxsim_create.restype = C.c_void_p
        L.apxsim_create.argtypes = [C.POINTER(capi.FlatIndexC)]
        L.apxsim_destroy.argtypes = [C.c_void_p]
        L.apxsim_run.restype = None
        L.apxsim_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.apxsim_fetch.restype = None
        L.apxsim_fetch.argtypes = [C.c_void_p] + [C.c_void_p] * 6
        _lib = L
    return _lib


class ApxSim:
    def __init__(self, fi, without_lcp=False):
        self.fi = fi
        st = capi.flat_struct(fi, without_lcp=without_lcp)
        self.h = sim_lib().apxsim_create(C.byref(st))
        if not self.h:
            raise RuntimeError("approx_sim: index rejected")

    def run(self, patterns, strands, k, max_hits, max_occ, chunk_len, max_steps):
        seq, offs = lm.ragged(patterns)
        seq = np.concatenate([seq, np.zeros(8, np.uint8)])
        prm = np.array([strands, k, max_hits, max_occ, chunk_len, max_steps], dtype=np.uint64)
        sizes = np.zeros(3, dtype=np.uint64)
        sim_lib().apxsim_run(self.h, seq.ctypes.data, offs.ctypes.data, len(patterns), prm.ctypes.data, sizes.ctypes.data)
        nt, nh, no = (int(x) for x in sizes)
        res, hits = np.zeros(nt + 1, dtype=am.RES_DTYPE), np.zeros(nh + 1, dtype=am.HIT_DTYPE)
        pos, sq, so = np.zeros(no + 1, dtype=np.uint64), np.zeros(no + 1, dtype=np.uint32), np.zeros(no + 1, dtype=np.uint64)
        cnt = np.zeros(4, dtype=np.uint64)
        sim_lib().apxsim_fetch(self.h, res.ctypes.data, hits.ctypes.data, pos.ctypes.data, sq.ctypes.data, so.ctypes.data, cnt.ctypes.data)
        return res[:-1], hits[:-1], pos[:-1], sq[:-1], so[:-1], cnt

    def close(self):
        if self.h:
            sim_lib().apxsim_destroy(self.h)
            self.h = None


def compare(got, want):
    """got: (res, hits, pos, seq, seq_off, counters) of the replay; want: ApproxModel.approx_batch's tuple"""
    res, hits, pos, sq, so, cnt = got
    for name, a, b in (("res", res, want[0]), ("hits", hits, want[1])):
        assert len(a) == len(b), name
        for f in a.dtype.names:
            assert np.array_equal(a[f], b[f]), (name, f, np.nonzero(np.atleast_1d(a[f] != b[f]))[0][:5])
    assert np.array_equal(pos, want[2]) and np.array_equal(sq, want[3]) and np.array_equal(so, want[4])
    assert int(cnt[0]) == want[5]                                # the steps of the search tree
    assert int(cnt[2]) == int((want[1]["n_occ"].astype(np.int64) - 1).clip(min=0).sum())


_models = {}


def check(fi, patterns, strands, k, max_hits, max_occ, chunk_len=16, max_steps=DEFAULT, without_lcp=False):
    sim = ApxSim(fi, without_lcp)
    try:
        model = _models.setdefault(id(fi), am.ApproxModel(fi))
        want = model.approx_batch(patterns, strands, k, max_hits, max_occ, chunk_len, max_steps)
        got = sim.run(patterns, strands, k, max_hits, max_occ, chunk_len, max_steps)
        compare(got, want)
        return got
    finally:
        sim.close()


@pytest.mark.parametrize("strands,k,max_hits,max_occ", [(1, 0, 0, 0), (1, 1, 8, 4), (2, 2, 64, 1000), (2, 3, 4, 1)])
def test_planted_case(strands, k, max_hits, max_occ):
    fi, text, pats, marks = am.approx_patterns()
    res, hits, pos, sq, so, cnt = check(fi, pats, strands, k, max_hits, max_occ)
    if max_hits:
        am.check_against_brute(text, pats, res, hits, pos, sq, so, strands, k, max_hits, max_occ, fi.seq_starts)
    assert int(res["complete"].min()) == 1
    assert int(cnt[3]) > 0                                       # N has no hot slot, the poly-A run is long: steps on the general path
    t = lambda name: marks[name] * strands
    assert int(res["n_hits"][t("empty")]) == 0 and int(res["cnt"][t("empty")].sum()) == 0
    assert int(res["cnt"][t("N against N"), 0]) >= 1 and int(res["cnt"][t("len 1"), 0]) >= 1
    for name in ("len 15", "len 16", "len 17"):                  # chunk_len - 1, chunk_len, chunk_len + 1
        assert int(res["cnt"][t(name), 0]) >= 1
    # the exact path dies in the first, a middle and the last of the three chunks of a 40-mer
    assert [int(res["matched"][t(n)]) for n in ("dies first", "dies middle", "dies last")] == [0, 19, 39]
    if k >= 1:
        for name in ("absent byte", "byte <= 1", "lower case", "dies first", "dies middle", "dies last"):      # each paid for as a mismatch
            assert int(res["cnt"][t(name), 0]) == 0 and int(res["cnt"][t(name), 1]) >= 1, name
        assert int(res["cnt"][t("N in pattern"), 1]) >= 1        # an N of the pattern against a letter of the text
    if k == 3:
        assert ((res["cnt"] > 0).all(axis=1)).any()              # a task with hits at every level 0..3
        assert (res["n_hits"] > max_hits).any() and int(res["n_kept"].max()) == max_hits


@pytest.mark.parametrize("chunk_len", [1, 7, 1 << 20, 0xFFFFFFFF])
def test_pieces(chunk_len):
    fi, text, pats, marks = am.approx_patterns()
    res, hits, pos, sq, so, cnt = check(fi, pats, 2, 2, 64, 3, chunk_len, 0)
    am.check_against_brute(text, pats, res, hits, pos, sq, so, 2, 2, 64, 3, fi.seq_starts)


def test_max_steps_stops_a_piece():
    fi, text, pats, marks = am.approx_patterns()
    full = check(fi, pats, 1, 2, 1 << 20, 0, 16, 0)[0]
    cut = check(fi, pats, 1, 2, 1 << 20, 0, 16, 40)[0]           # (equal to the model's, bound included: check() compared them)
    stopped = cut["complete"] == 0
    assert stopped.any() and not stopped.all()
    assert (cut["cnt"] <= full["cnt"]).all() and (cut["n_hits"] <= full["n_hits"]).all() and (cut["n_hits"][stopped] < full["n_hits"][stopped]).any()
    assert np.array_equal(cut["cnt"][~stopped], full["cnt"][~stopped])


def test_without_lcp_samples():
    fi, text, pats, marks = am.approx_patterns()
    res, hits, pos, sq, so, cnt = check(fi, pats, 2, 1, 16, 2, without_lcp=True)
    am.check_against_brute(text, pats, res, hits, pos, sq, so, 2, 1, 16, 2, fi.seq_starts)


def test_standalone_program_under_sanitizers(tmp_path):
    """the same per-lane code in a program of its own, compiled with -fsanitize=address,undefined and run as a child process on the planted case:
    it must end clean and give the model's values (the sanitizers' runtimes are linked statically: the program needs nothing from its environment)"""
    exe = os.path.join(HERE, "approx_sim_asan")
    if stale(exe):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                               "-DAPPROX_SIM_MAIN", "-o", exe, SRC])
    fi, text, pats, marks = am.approx_patterns()
    model = _models.setdefault(id(fi), am.ApproxModel(fi))
    for strands, k, max_hits, max_occ, chunk_len, max_steps, with_lcp in ((2, 3, 4, 2, 16, DEFAULT, 1), (1, 2, 64, 5, 7, 40, 0), (2, 1, 0, 0, 1, 0, 1)):
        seq, offs = lm.ragged(pats)
        n_seq = len(fi.seq_starts) - 1
        u64 = lambda a: np.ascontiguousarray(a, dtype=np.uint64).tobytes()
        blob = u64([fi.n, fi.r, fi.w, n_seq, with_lcp, len(pats), strands, k, max_hits, max_occ, chunk_len, max_steps, 0, 0]) + u64(fi.F) + u64(fi.starts) + u64(fi.ssa) + u64(fi.esa)
        blob += u64(fi.thr) + (u64(fi.slcp) if with_lcp else b"") + u64(fi.seq_starts) + u64(offs) + np.ascontiguousarray(fi.heads, dtype=np.uint8).tobytes() + seq.tobytes()
        src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
        src.write_bytes(blob)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([exe, str(src), str(dst)], env=env, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-2000:]
        raw = dst.read_bytes()
        head = np.frombuffer(raw[:64], dtype=np.uint64)
        nt, nh, no = (int(x) for x in head[:3])
        assert nt == len(pats) * strands and len(raw) == 64 + nt * 64 + nh * 40 + no * 20
        at = 64
        res = np.frombuffer(raw[at:at + nt * 64], dtype=am.RES_DTYPE); at += nt * 64
        hits = np.frombuffer(raw[at:at + nh * 40], dtype=am.HIT_DTYPE); at += nh * 40
        pos = np.frombuffer(raw[at:at + no * 8], dtype=np.uint64); at += no * 8
        so = np.frombuffer(raw[at:at + no * 8], dtype=np.uint64); at += no * 8
        sq = np.frombuffer(raw[at:at + no * 4], dtype=np.uint32)
        compare((res, hits, pos, sq, so, head[3:7]), model.approx_batch(pats, strands, k, max_hits, max_occ, chunk_len, max_steps))
