"""screen_task (moni_align_amd/csrc/screen_core.h: what screen_kernel runs per lane) replayed on the host over the device index image, against
the plain-Python definition of tests/screen_model.py, record for record and with no tolerance; the walk takes 2 * strands steps per base, and the
lanes of strand 0's pattern take the threshold jumps of PmlModel.walk.  The real kernel is checked the same way under -m gpu."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from moni_align_amd import capi
from tests import pml_model, screen_model as sm
from tests.test_host_sim import long_run_case

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sim")
_lib = None

PARAM_SETS = (sm.Params(), sm.Params(64, 32, 1, 2), sm.Params(8, 1, 1, 1))


def sim_lib():
    """tests/host_sim/libscreen_sim.so, built beside the host-sim library and leaving it alone"""
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "libscreen_sim.so")
        src = os.path.join(HERE, "screen_sim.cpp")
        deps = [src] + [os.path.join(capi.CSRC, f) for f in ("screen_core.h", "pml_core.h", "seed_core.h", "image.hpp", "layout.h")]
        deps.append(os.path.join(os.path.dirname(capi.HERE), "include", "moni_hip.h"))
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", so, src])
        L = C.CDLL(so)
        L.screensim_create.restype = C.c_void_p
        L.screensim_create.argtypes = [C.POINTER(capi.FlatIndexC)]
        L.screensim_destroy.argtypes = [C.c_void_p]
        L.screensim_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(capi.ScreenParamsC), C.c_void_p, C.c_void_p]
        L.screensim_n_win.argtypes = [C.c_uint32, C.POINTER(capi.ScreenParamsC)]
        L.screensim_n_win.restype = C.c_uint32
        _lib = L
    return _lib


def params_c(p: sm.Params) -> capi.ScreenParamsC:
    c = capi.ScreenParamsC()
    c.window, c.min_win, c.ks_num, c.ks_den, c.strands = p
    return c


class ScreenSim:
    def __init__(self, fi):
        st = capi.flat_struct(fi)
        self.h = sim_lib().screensim_create(C.byref(st))
        if not self.h:
            raise RuntimeError("screen_sim: index rejected")

    def run(self, reads, p: sm.Params):
        seq, offs = pml_model.ragged(reads)
        n = len(reads)
        res = np.zeros(n + 1, dtype=capi.SCREEN_RES_DTYPE)
        cnt = np.zeros(4, dtype=np.uint64)
        seq = np.concatenate([seq, np.zeros(8, np.uint8)])
        pc = params_c(p)
        rc = sim_lib().screensim_run(self.h, seq.ctypes.data, offs.ctypes.data, n, C.byref(pc), res.ctypes.data, cnt.ctypes.data)
        assert rc == 0
        return res[:-1], cnt

    def close(self):
        if self.h:
            sim_lib().screensim_destroy(self.h)
            self.h = None


def check(fi, reads, param_sets=PARAM_SETS):
    """both strands settings under every parameter set; returns the model's records of the first set, two strands"""
    model = pml_model.PmlModel(fi)
    sim = ScreenSim(fi)
    try:
        walked = [sm.walk_read(model, r) for r in reads]
        jumps_p0 = sum(model.walk(r)[1] for r in reads)
        total = sum(len(r) for r in reads)
        first = None
        for p0 in param_sets:
            for strands in (2, 1):
                p = p0._replace(strands=strands)
                want = [sm.screen_read(model, r, p, walked=w) for r, w in zip(reads, walked)]
                res, cnt = sim.run(reads, p)
                got = sm.as_tuples(res)
                for i, (g, w) in enumerate(zip(got, want)):
                    assert g == w, "read %d (length %d) %r: got %r want %r" % (i, len(reads[i]), p, g, w)
                assert int(cnt[0]) == 2 * strands * total          # one step per base and string
                assert int(cnt[2]) == jumps_p0                     # strand 0's pattern lanes jump where the model's walk does
                assert int(cnt[1]) >= int(cnt[2]) and int(cnt[3]) == 0      # every histogram column left zero, every traded value taken
                first = first or want
        return first
    finally:
        sim.close()


def ragged_lengths(case):
    """reads cut at the pattern-word, window and min_win edges"""
    base = [r.tobytes() for r in case.synth.make_reads(case.pg, 3, 300, seed=71, sub_rate=0.02, indel_rate=0.0005)]
    return [base[k % 3][:L] for k, L in enumerate((0, 1, 7, 8, 9, 24, 25, 49, 50, 51, 63, 64, 65, 74, 75, 100, 255, 256, 257, 300))]


def test_simulated_reads_medium(medium_case):
    reads = pml_model.sim_reads(medium_case) + ragged_lengths(medium_case)
    want = check(medium_case.fi, reads)
    assert sm.n_present(want) >= 20 and any(r[4] & sm.STRAND1 for r in want) and any(r[4] & sm.SHORT for r in want)


def test_long_runs_and_cold_letters():
    """runs past the 12-bit length field, a letter without a hot slot (N occurs in this BWT), the general path"""
    fi, reads = long_run_case()
    want = check(fi, [r.tobytes() for r in reads[:120]], param_sets=PARAM_SETS[:2])
    assert sm.n_present(want) >= 60


def test_n_win_and_parameter_ranges():
    L = sim_lib()
    for p in PARAM_SETS + (sm.Params(65535, 1), sm.Params(150, 150)):
        pc = params_c(p)
        for m in (0, 1, p.min_win - 1, p.min_win, p.window - 1, p.window, p.window + p.min_win - 1, p.window + p.min_win, 2 * p.window, 1000003):
            assert L.screensim_n_win(m, C.byref(pc)) == len(sm.windows(m, p)), (p, m)
    fi, reads = long_run_case()
    sim = ScreenSim(fi)
    try:
        seq, offs = pml_model.ragged([reads[0].tobytes()])
        res, cnt = np.zeros(2, dtype=capi.SCREEN_RES_DTYPE), np.zeros(4, dtype=np.uint64)
        for bad in (sm.Params(window=7), sm.Params(window=65536), sm.Params(min_win=0), sm.Params(min_win=51), sm.Params(ks_num=0), sm.Params(ks_num=5),
                    sm.Params(ks_num=1, ks_den=65536), sm.Params(strands=0), sm.Params(strands=3)):
            pc = params_c(bad)
            assert L.screensim_run(sim.h, seq.ctypes.data, offs.ctypes.data, 1, C.byref(pc), res.ctypes.data, cnt.ctypes.data) == -22, bad
    finally:
        sim.close()
