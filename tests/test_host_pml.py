"""pml_task (moni_align_amd/csrc/pml_core.h: what pml_kernel runs per lane) replayed on the host over the device index image, against the
plain-Python model of tests/pml_model.py: lengths, read_max and read_hits, no tolerance; and its walk takes the steps and the threshold jumps
of the pointer walk (ms_task) over strand 0 of the same reads.  The real kernel is checked the same way under -m gpu."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from moni_align_amd import capi
from tests import pml_model
from tests.test_host_sim import long_run_case

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sim")
_lib = None


def sim_lib():
    """tests/host_sim/libpml_sim.so, built beside the host-sim library and leaving it alone"""
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "libpml_sim.so")
        src = os.path.join(HERE, "pml_sim.cpp")
        deps = [src] + [os.path.join(capi.CSRC, f) for f in ("pml_core.h", "seed_core.h", "image.hpp", "layout.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", so, src])
        L = C.CDLL(so)
        L.pmlsim_create.restype = C.c_void_p
        L.pmlsim_create.argtypes = [C.POINTER(capi.FlatIndexC)]
        L.pmlsim_destroy.argtypes = [C.c_void_p]
        L.pmlsim_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32] + [C.c_void_p] * 4
        _lib = L
    return _lib


class PmlSim:
    def __init__(self, fi):
        self.fi = fi
        st = capi.flat_struct(fi)
        self.h = sim_lib().pmlsim_create(C.byref(st))
        if not self.h:
            raise RuntimeError("pml_sim: index rejected")

    def run(self, reads, thr=25):
        seq, offs = pml_model.ragged(reads)
        n = len(reads)
        ln = np.zeros(len(seq) + 1, dtype=np.uint32)
        mx = np.zeros(n + 1, dtype=np.uint32)
        hits = np.zeros(n + 1, dtype=np.uint32)
        cnt = np.zeros(4, dtype=np.uint64)
        seq = np.concatenate([seq, np.zeros(8, np.uint8)])
        rc = sim_lib().pmlsim_run(self.h, seq.ctypes.data, offs.ctypes.data, n, thr, ln.ctypes.data, mx.ctypes.data, hits.ctypes.data, cnt.ctypes.data)
        assert rc == 0
        return ln[:-1], mx[:-1], hits[:-1], cnt

    def close(self):
        if self.h:
            sim_lib().pmlsim_destroy(self.h)
            self.h = None


def check(fi, reads, thrs=(25,)):
    model = pml_model.PmlModel(fi)
    sim = PmlSim(fi)
    try:
        walks = [model.walk(r) for r in reads]
        for thr in thrs:
            want_ln, want_mx, want_hits = model.batch(reads, thr)
            ln, mx, hits, cnt = sim.run(reads, thr)
            assert np.array_equal(ln, want_ln)
            assert np.array_equal(mx, want_mx)
            assert np.array_equal(hits, want_hits)
            total = sum(len(r) for r in reads)
            assert int(cnt[0]) == total and int(cnt[2]) == total          # one step per base, in both walks
            assert int(cnt[1]) == int(cnt[3])                             # the same threshold jumps as the pointer walk of strand 0
            assert int(cnt[1]) == sum(j for _, j in walks)                # ... and as the model
        return want_ln
    finally:
        sim.close()


def test_simulated_reads_medium(medium_case):
    reads = pml_model.sim_reads(medium_case)
    ln = check(medium_case.fi, reads, thrs=(25, 1, 10000))
    assert int((ln >= 25).sum()) * 10 >= len(ln)


def test_long_runs_and_cold_letters():
    """runs past the 12-bit length field, a letter without a hot slot (N occurs in this BWT), the general path: all 400 reads"""
    fi, reads = long_run_case()
    ln = check(fi, [r.tobytes() for r in reads])
    assert int(ln.max()) >= 25
