"""The three per-lane routines of moni_align_amd/csrc/mslong_core.h (the segment cuts, mslong_walk, mslong_len: what the kernels of
moni_ms_long_batch run per lane) replayed on the host over the device index image, lanes as loops, against OracleIndex.ms_lengths: the lengths
at every position, the validity of every pointer, and the step counts, no tolerance (tests/mslong_model.py has the checks and the patterns).
The real kernels are checked the same way under -m gpu (tests/test_gpu_mslong.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from moni_align_amd import capi
from tests import mslong_model as mm
from tests.test_host_sim import long_run_case

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sim")
_lib = None


def sim_lib():
    """tests/host_sim/libmslong_sim.so, built beside the host-sim library and leaving it alone"""
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "libmslong_sim.so")
        src = os.path.join(HERE, "mslong_sim.cpp")
        deps = [src] + [os.path.join(capi.CSRC, f) for f in ("mslong_core.h", "seed_core.h", "image.hpp", "layout.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", so, src])
        L = C.CDLL(so)
        L.mslsim_create.restype = C.c_void_p
        L.mslsim_create.argtypes = [C.POINTER(capi.FlatIndexC)]
        L.mslsim_destroy.argtypes = [C.c_void_p]
        L.mslsim_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        _lib = L
    return _lib


class MslSim:
    def __init__(self, fi):
        self.fi = fi
        st = capi.flat_struct(fi)
        self.h = sim_lib().mslsim_create(C.byref(st))
        if not self.h:
            raise RuntimeError("mslong_sim: index rejected")
        self.segs = None

    def __call__(self, seq, offs, seg_len, overlap):
        total, n = int(offs[-1] - offs[0]), len(offs) - 1
        ptr = np.full(total + 1, 2 ** 63, dtype=np.uint64)           # a place the replay does not write shows
        ln = np.full(total + 1, 0xFFFFFFFF, dtype=np.uint32)
        st = np.zeros(6, dtype=np.uint64)
        cap = total + n + 1
        segs = np.zeros((cap, 4), dtype=np.uint32)
        seq = np.concatenate([np.ascontiguousarray(seq, dtype=np.uint8), np.zeros(8, np.uint8)])
        rc = sim_lib().mslsim_run(self.h, seq.ctypes.data, np.ascontiguousarray(offs, dtype=np.uint64).ctypes.data, n, seg_len, overlap, ptr.ctypes.data, ln.ctypes.data,
                                  st.ctypes.data, segs.ctypes.data, cap)
        assert rc == 0
        assert int(ptr[-1]) == 2 ** 63 and int(ln[-1]) == 0xFFFFFFFF          # nothing behind the batch was touched
        self.segs = [tuple(int(x) for x in r) for r in segs[:int(st[0])]]
        keys = ("segments", "flagged", "chain_runs", "steps_spec", "steps_chain", "jumps")
        return ptr[:-1], ln[:-1], dict(zip(keys, (int(v) for v in st)))

    def close(self):
        if self.h:
            sim_lib().mslsim_destroy(self.h)
            self.h = None


@pytest.fixture(scope="module")
def rig(medium_case):
    from oracle import orc
    sim = MslSim(medium_case.fi)
    yield sim, orc.OracleIndex(medium_case.path), medium_case.text, int(medium_case.fi.n)
    sim.close()


@pytest.fixture(scope="module")
def random_want(rig):
    pats = mm.random_batch()
    return pats, [rig[1].ms_lengths(p) for p in pats]


def test_cuts_model():
    """the plain-Python cuts: segments tile the pattern, none is longer than seg_len, all but the first begin at a multiple of 8 of the output index"""
    for seg_len, overlap in mm.SETTINGS + [(13, 5), (4095, 7)]:
        for g0 in (0, 1, 5, 7, 8, 1003):
            for m in mm.edge_lengths(seg_len) + [20000]:
                cs = mm.cuts(g0, m, seg_len, overlap)
                assert [a for a, _, _ in cs[1:]] == [b for _, b, _ in cs[:-1]]
                assert (not cs and m == 0) or (cs[0][0] == 0 and cs[-1][1] == m and cs[-1][2] == m)
                assert all(0 < b - a <= seg_len and e == min(b + overlap, m) for a, b, e in cs)
                assert all((g0 + a) % 8 == 0 for a, _, _ in cs[1:])
                assert len(cs) <= 1 or m > seg_len


@pytest.mark.parametrize("seg_len,overlap", mm.SETTINGS)
def test_ragged_batch(rig, medium_case, seg_len, overlap):
    """(c) + (d): edge lengths, a 20 000-base pattern, N / lower case / an absent byte at segment edges and inside an overlap; ragged offsets"""
    sim, orc_idx, text, n = rig
    pats = mm.ragged_batch(medium_case, seg_len, overlap)
    st, (tab, flags, runs), want = mm.check(sim, orc_idx, text, n, pats, seg_len, overlap)
    assert sim.segs == tab                                           # the header's cuts are the model's
    assert st["flagged"] > 0 and max(int(w[1].max()) for w in want if len(w[1])) >= 100
    assert all(int(w[1][k]) == 0 for p, w in zip(pats[-5:-1], want[-5:-1]) for k in range(len(p)) if p[k:k + 1] not in (b"A", b"C", b"G", b"T"))
    assert not want[-1][1].any()
    if seg_len < 4096:
        assert mm.odd_starts(pats, want, n, seg_len, overlap) >= 1           # a length carried across a cut was needed
    mm.check(sim, orc_idx, text, n, pats[::-1], seg_len, overlap, want[::-1])          # other offsets, other groups of 8


@pytest.mark.parametrize("seg_len,overlap", mm.SETTINGS)
def test_random_patterns(rig, random_want, seg_len, overlap):
    """(a): matches are short, so with an overlap of 16 and more no segment is flagged - confirmed from the oracle's lengths by mm.check's prediction"""
    sim, orc_idx, text, n = rig
    pats, want = random_want
    st, (tab, flags, runs), _ = mm.check(sim, orc_idx, text, n, pats, seg_len, overlap, want)
    if overlap >= 16:
        assert max(int(w[1].max()) for w in want) <= 16 and not any(flags)          # the condition, from the oracle's lengths: no match reaches across an overlap of 16
        assert st["flagged"] == 0 and st["chain_runs"] == 0 and st["steps_chain"] == 0


@pytest.mark.parametrize("seg_len,overlap", mm.SETTINGS)
def test_substring_is_one_chain(rig, medium_case, seg_len, overlap):
    """(b): every segment but the last is flagged and one lane walks them all"""
    sim, orc_idx, text, n = rig
    p = mm.substring_pattern(medium_case, seg_len)
    st, _, want = mm.check(sim, orc_idx, text, n, [p], seg_len, overlap)
    assert st["segments"] >= 10 and st["flagged"] == st["segments"] - 1 and st["chain_runs"] == 1
    assert int(want[0][1][0]) == len(p)


@pytest.mark.parametrize("seg_len,overlap", mm.SETTINGS)
def test_haplotype_is_mixed(rig, medium_case, seg_len, overlap):
    """(c): a whole haplotype with a substitution every ~300 bases.  With an overlap of 0 a segment is flagged as soon as its last base occurs in the
    text at all, so every segment but the last is, and they are one run; the mixed outcome is asserted where the overlap can tell (16 and more)."""
    sim, orc_idx, text, n = rig
    p = mm.haplotype_pattern(medium_case)
    st, _, _ = mm.check(sim, orc_idx, text, n, [p], seg_len, overlap)
    assert 0 < st["flagged"] < st["segments"]
    if overlap >= 16:
        assert st["chain_runs"] > 1
    if overlap == 0:
        assert st["flagged"] == st["segments"] - 1 and st["chain_runs"] == 1


def test_uncut_is_the_reference_walk(rig, medium_case):
    """seg_len >= the longest pattern: one segment per pattern, nothing flagged, pointers equal to the oracle's (checked inside mm.check)"""
    sim, orc_idx, text, n = rig
    pats = mm.ragged_batch(medium_case, 64, 16)
    st, _, _ = mm.check(sim, orc_idx, text, n, pats, 1 << 20, 256)
    assert st["segments"] == sum(1 for p in pats if p) and st["flagged"] == 0 and st["steps_spec"] == sum(len(p) for p in pats)


@pytest.fixture(scope="module")
def long_runs(tmp_path_factory):
    from oracle import orc
    fi, reads = long_run_case()
    path = str(tmp_path_factory.mktemp("mslong") / "long_runs.mfi")
    fi.save(path)
    text = fi.text.tobytes()
    pats = [r.tobytes() for r in reads[:60]]
    rng = np.random.default_rng(21)
    for at, L in ((500, 9000), (33000 - 20, 5000), (100000, 12001)):          # long windows of the text with a few errors, across the N blocks
        w = np.frombuffer(text[at:at + L], dtype=np.uint8).copy()
        for e in rng.integers(0, L, size=L // 700):
            w[int(e)] = mm.ACGT[int(rng.integers(0, 4))]
        pats.append(w.tobytes())
    o = orc.OracleIndex(path)
    sim = MslSim(fi)
    yield sim, o, text, int(fi.n), pats, [o.ms_lengths(p) for p in pats]
    sim.close()


@pytest.mark.parametrize("seg_len,overlap", mm.SETTINGS)
def test_long_runs_and_cold_letters(long_runs, seg_len, overlap):
    """(e): runs past the 12-bit length field, a letter without a hot slot (N occurs in this BWT), the general path"""
    sim, orc_idx, text, n, pats, want = long_runs
    st, _, _ = mm.check(sim, orc_idx, text, n, pats, seg_len, overlap, want)
    assert max(int(w[1].max()) for w in want) >= 150 and st["jumps"] > 0
