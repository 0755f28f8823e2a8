"""loc_task / loc_walk (moni_align_amd/csrc/locate_core.h: what count_kernel and locate_walk_kernel run per lane) replayed on the host over the
device index image, against the plain-Python model of tests/locate_model.py: every field of every record and every position, no tolerance.  The
real kernels are checked against brute force under -m gpu."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from moni_align_amd import capi
from tests import locate_model as lm
from tests.test_host_sim import long_run_case

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sim")
_lib = None


def sim_lib():
    """tests/host_sim/liblocate_sim.so, built beside the host-sim library and leaving it alone"""
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "liblocate_sim.so")
        src = os.path.join(HERE, "locate_sim.cpp")
        deps = [src] + [os.path.join(capi.CSRC, f) for f in ("locate_core.h", "seed_core.h", "image.hpp", "layout.h")] + [os.path.join(os.path.dirname(capi.HERE), "include", "moni_hip.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", so, src])
        L = C.CDLL(so)
        L.locsim_create.restype = C.c_void_p
        L.locsim_create.argtypes = [C.POINTER(capi.FlatIndexC)]
        L.locsim_destroy.argtypes = [C.c_void_p]
        L.locsim_run.restype = C.c_uint64
        L.locsim_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.locsim_fetch.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


class LocSim:
    def __init__(self, fi, without_lcp=False):
        self.fi = fi
        st = capi.flat_struct(fi, without_lcp=without_lcp)
        self.h = sim_lib().locsim_create(C.byref(st))
        if not self.h:
            raise RuntimeError("locate_sim: index rejected")

    def run(self, patterns, strands=1, max_occ=0):
        seq, offs = lm.ragged(patterns)
        n = len(patterns)
        res = np.zeros(n * strands + 1, dtype=lm.RES_DTYPE)
        cnt = np.zeros(4, dtype=np.uint64)
        seq = np.concatenate([seq, np.zeros(8, np.uint8)])
        k = sim_lib().locsim_run(self.h, seq.ctypes.data, offs.ctypes.data, n, strands, max_occ, res.ctypes.data, cnt.ctypes.data)
        pos, sq, so = np.zeros(k, np.uint64), np.zeros(k, np.uint32), np.zeros(k, np.uint64)
        sim_lib().locsim_fetch(self.h, k, pos.ctypes.data, sq.ctypes.data, so.ctypes.data)
        return res[:-1], pos, sq, so, cnt

    def close(self):
        if self.h:
            sim_lib().locsim_destroy(self.h)
            self.h = None


def check(fi, patterns, strands, max_occ, without_lcp=False):
    model = lm.LocateModel(fi)
    sim = LocSim(fi, without_lcp)
    try:
        want = model.batch(patterns, strands, max_occ)
        res, pos, sq, so, cnt = sim.run(patterns, strands, max_occ)
        for k in lm.RES_DTYPE.names:
            assert np.array_equal(res[k], want[0][k]), (k, np.nonzero(res[k] != want[0][k])[0][:5])
        assert np.array_equal(pos, want[1]) and np.array_equal(sq, want[2]) and np.array_equal(so, want[3])
        # a step is counted for every byte that reaches the index: the bytes matched, and the one the search dies at unless it is not a letter of the BWT
        present = set(int(x) for x in np.unique(fi.heads))
        steps = 0
        for i, p in enumerate(patterns):
            for s in range(strands):
                q = lm.revcomp(p) if s else p
                mt = int(res["matched"][i * strands + s])
                steps += mt + (1 if mt < len(q) and q[len(q) - 1 - mt] in present and q[len(q) - 1 - mt] > 1 else 0)
        assert int(cnt[0]) == steps
        assert int(cnt[1]) <= 2 * steps + int(cnt[0])          # at most two rows per step beside the walks over runs the LF image ran past
        assert int(cnt[2]) == int((res["n_occ"].astype(np.int64) - 1).clip(min=0).sum())
        return res, cnt
    finally:
        sim.close()


@pytest.mark.parametrize("strands,max_occ", [(1, 0), (2, 4), (2, 100000)])
def test_planted_case(strands, max_occ):
    fi, text, pats = lm.planted_case()
    res, cnt = check(fi, pats, strands, max_occ)
    assert int(res["count"].max()) >= 100 and int((res["count"] > 0).sum()) >= 20
    assert int(cnt[3]) > 0                                       # N has no hot slot: the general path was taken


def test_without_lcp_samples():
    fi, text, pats = lm.planted_case()
    check(fi, pats, 2, 7, without_lcp=True)


def test_simulated_reads_and_their_pieces(medium_case):
    reads = [r.tobytes() for r in medium_case.synth.make_reads(medium_case.pg, 60, 150, seed=71, sub_rate=0.01)]
    pats = reads + [r[40:72] for r in reads] + [r[:k] for k, r in enumerate(reads)]
    res, cnt = check(medium_case.fi, pats, 2, 16)
    assert int((res["count"] > 0).sum()) >= 90                     # of 360 tasks: most forward 32-mers and prefixes occur, few whole reads, few reverse strands
    assert int(cnt[1]) < 2 * int(cnt[0])                         # the ends share a run often enough to show


def test_long_runs_and_cold_letters():
    """runs past the 12-bit length field, a letter without a hot slot (N occurs in this BWT), the general path"""
    fi, reads = long_run_case()
    reads = [r.tobytes() for r in reads]
    text = fi.text.tobytes()
    pats = [r[100:130] for r in reads[:150]] + reads[:20] + [text[a:a + 60] for a in range(0, 60000, 1500)] + [b"C" + text[13:53], b"N", b"NNNN", b"ANNNN", text[12:53]]
    res, cnt = check(fi, pats, 2, 8)
    assert int(cnt[3]) > 0 and int(res["count"].max()) >= 4095
