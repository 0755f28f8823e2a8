"""cov_core.h (what the kernels of the depth of coverage run per record, slot, line and window) replayed on the host - lanes as loops, passes in
launch order, elements last to first - against tests/coverage_model byte for byte: the stats of an add, the figures of the seal, the
per-base text at every window of the grid, the window sums.  The bad-record classes of the sort give their reasons and the lowest index, and
add nothing.  The real kernels are held to the same model under -m gpu (tests/test_gpu_coverage.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from moni_align_amd import capi
from tests import bam_model as bam
from tests import coverage_model as cm
from tests.bamsort_cases import BAD, GOOD, REASONS, bad_batch, offsets
from tests.coverage_cases import BASES_GRID, H_ONE, HDR, LINES_GRID, WINDOWS, cases

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sim")
EINVAL, ERANGE = -22, -34
COV_REF_DTYPE = np.dtype([("length", np.uint64), ("bases", np.uint64), ("min", np.uint32), ("max", np.uint32)])
STAT_NAMES = ("records", "counted", "skipped_flag", "skipped_mapq", "unplaced", "clipped", "blocks", "bad_records", "first_bad_record", "bad_reason")
_lib = None


def sim_lib():
    """tests/host_sim/libcoverage_sim.so, built beside the other host-sim libraries and leaving them alone"""
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "libcoverage_sim.so")
        src = os.path.join(HERE, "coverage_sim.cpp")
        deps = [src] + [os.path.join(capi.CSRC, f) for f in ("cov_core.h", "render_core.h", "bam_sort_core.h", "bam_core.h")] + [os.path.join(os.path.dirname(capi.HERE), "include", "moni_hip.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
        L = C.CDLL(so)
        L.covsim_create.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        L.covsim_create.restype = C.c_void_p
        L.covsim_destroy.argtypes = [C.c_void_p]
        L.covsim_destroy.restype = None
        L.covsim_set_counted.argtypes = [C.c_void_p, C.c_uint64]
        L.covsim_set_counted.restype = None
        L.covsim_add.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
        L.covsim_seal.argtypes = [C.c_void_p, C.c_void_p]
        L.covsim_next.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        L.covsim_windows.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        _lib = L
    return _lib


class Sim:
    """one object of the replay over the dictionary of `header`"""

    def __init__(self, header, exclude=cm.EXCLUDE, min_mapq=0):
        refs = bam.references(header)
        ln = np.array([l for _, l in refs], np.uint64)
        names = np.frombuffer(b"".join(n for n, _ in refs) + b"\0", np.uint8)
        off = np.concatenate([[0], np.cumsum([len(n) for n, _ in refs])]).astype(np.uint32)
        self.n_ref = len(refs)
        self.h = sim_lib().covsim_create(ln.ctypes.data, len(refs), names.ctypes.data, off.ctypes.data, exclude, min_mapq)

    def add(self, recs, off=None, trusted=False):
        data = np.frombuffer(recs if isinstance(recs, bytes) else b"".join(recs), dtype=np.uint8)
        off = offsets(recs) if off is None else np.ascontiguousarray(off, np.uint64)
        st = np.zeros(10, np.uint64)
        rc = sim_lib().covsim_add(self.h, data.ctypes.data if data.size else None, data.size, off.ctypes.data, len(off) - 1, int(trusted), st.ctypes.data)
        return rc, dict(zip(STAT_NAMES, (int(x) for x in st)))

    def seal(self):
        refs = np.zeros(max(self.n_ref, 1), COV_REF_DTYPE)
        rc = sim_lib().covsim_seal(self.h, refs.ctypes.data)
        return rc, [tuple(int(x) for x in r) for r in refs[:self.n_ref]]

    def next(self, max_bases, max_lines):
        t, n, done = C.c_void_p(), C.c_uint64(), C.c_int()
        rc = sim_lib().covsim_next(self.h, max_bases, max_lines, C.byref(t), C.byref(n), C.byref(done))
        return rc, (C.string_at(t.value, n.value) if n.value else b""), done.value

    def text(self, max_bases, max_lines):
        out, calls = [], 0
        while True:
            rc, piece, done = self.next(max_bases, max_lines)
            assert rc == 0
            assert piece.count(b"\n") <= max_lines and (not piece or piece.endswith(b"\n"))
            out.append(piece)
            calls += 1
            assert calls < 100000
            if done:
                return b"".join(out)

    def windows(self, r, w):
        p, n = C.c_void_p(), C.c_uint64()
        rc = sim_lib().covsim_windows(self.h, r, w, C.byref(p), C.byref(n))
        return rc, (np.frombuffer(C.string_at(p.value, 8 * n.value), np.uint64).tolist() if rc == 0 and n.value else [])

    def close(self):
        if self.h:
            sim_lib().covsim_destroy(self.h)
            self.h = None

    __del__ = close


CASES = cases()
MODELS = {name: cm.Coverage(HDR, min_mapq=q).add(recs) for name, recs, q in CASES}          # computed once, read by every test


def model_stats(m):
    return dict(m.stats, bad_records=0, first_bad_record=0, bad_reason=0)


@pytest.mark.parametrize("name,recs,mapq", CASES, ids=[c[0] for c in CASES])
def test_replay_matches_model(name, recs, mapq):
    m = MODELS[name]
    s = Sim(HDR, min_mapq=mapq)
    rc, st = s.add(recs)
    assert rc == 0 and st == model_stats(m)
    rc, refs = s.seal()
    assert rc == 0 and refs == m.ref_figures()
    assert s.add(recs)[0] == EINVAL, "an add after the seal"
    assert s.text(1 << 20, 1 << 20) == m.per_base()
    for r in range(3):
        for w in WINDOWS:
            assert s.windows(r, w) == (0, m.windows(r, w))
    assert s.windows(3, 1)[0] == EINVAL and s.windows(0, 0)[0] == EINVAL and s.windows(0, 1 << 31)[0] == EINVAL


@pytest.mark.parametrize("name", ["edges", "cigars", "pile257", "boundary", "empty_ref", "random3000"])
def test_text_is_the_same_at_every_window(name):
    """where a wrong carry shows: every max_bases crossed with every max_lines"""
    recs, mapq = next((r, q) for n, r, q in CASES if n == name)
    want = MODELS[name].per_base()
    for mb in BASES_GRID:
        for ml in LINES_GRID:
            s = Sim(HDR, min_mapq=mapq)
            assert s.add(recs)[0] == 0 and s.seal()[0] == 0
            assert s.text(mb, ml) == want, (mb, ml)
            assert s.next(mb, ml) == (0, b"", 1), "behind the last piece"


def test_adds_in_parts_and_trusted():
    name, recs, mapq = next(c for c in CASES if c[0] == "random3000")
    s = Sim(HDR)
    assert s.add(recs[:1000])[0] == 0 and s.add(recs[1000:1001])[0] == 0 and s.add([])[0] == 0 and s.add(recs[1001:], trusted=True)[0] == 0
    assert s.seal()[1] == MODELS[name].ref_figures()
    assert s.text(64, 3) == MODELS[name].per_base()


def test_next_before_seal_and_bad_arguments():
    s = Sim(HDR)
    assert s.next(1, 1)[0] == EINVAL and s.windows(0, 1)[0] == EINVAL
    s.seal()
    assert s.next(0, 1)[0] == EINVAL and s.next(1, 0)[0] == EINVAL


def test_other_exclude():
    name, recs, _ = next(c for c in CASES if c[0] == "flags")
    s = Sim(HDR, exclude=0x304)
    s.add(recs)
    s.seal()
    want = cm.Coverage(HDR, exclude=0x304).add(recs)
    assert s.text(7, 2) == want.per_base() != MODELS[name].per_base()


@pytest.mark.parametrize("bad", BAD, ids=[b[0] for b in BAD])
def test_bad_record_adds_nothing(bad):
    data, off = bad_batch(bad)
    s = Sim(H_ONE)
    rc, st = s.add(data, off)
    assert rc == EINVAL and st["bad_records"] >= 1 and st["first_bad_record"] == 5 and REASONS[st["bad_reason"]] == bad[2]
    data2, off2 = bad_batch(bad, at=6, second=BAD[3], second_at=2)
    rc, st = s.add(data2, off2)
    assert rc == EINVAL and st["first_bad_record"] == 2 and REASONS[st["bad_reason"]] == BAD[3][2], "the lowest index"
    assert s.add(GOOD[:2])[1]["counted"] == 2
    m = cm.Coverage(H_ONE).add(GOOD[:2])
    assert s.seal()[1] == m.ref_figures(), "nothing of the bad calls was added"


def test_length_mismatch():
    s = Sim(H_ONE)
    off = offsets(GOOD)
    rc, st = s.add(b"".join(GOOD) + b"x", off)
    assert rc == EINVAL and st["first_bad_record"] == len(GOOD) and REASONS[st["bad_reason"]] == "LENGTH"


def test_limit():
    s = Sim(HDR)
    recs = [c for c in CASES if c[0] == "pile65"][0][1]
    sim_lib().covsim_set_counted(s.h, cm.LIMIT - 66)
    assert s.add(recs)[0] == 0, "2^31 - 1 counted records"
    assert s.add(recs[:1])[0] == ERANGE
    assert s.add([c for c in CASES if c[0] == "cigars"][0][1][-3:])[0] == 0, "records that do not count still pass"
    assert s.seal()[1] == MODELS["pile65"].ref_figures(), "the refused call added nothing"
