"""bam_dup_core.h (what the kernels of duplicate marking run per record, unit and entry) replayed on the host - lanes as loops, passes in launch
order, elements last to first - against tests/markdup_model byte for byte: the entries of every run, the marks of the resolve, and the records
that leave the marked sort.  Every new class of bad record gives its reason and the lowest index; an idx outside its run is refused.  The
real kernels are held to the replay's bytes under -m gpu (tests/test_gpu_markdup.py)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from moni_align_amd import capi
from tests import bam_model as bam
from tests import bamsort_model as bsm
from tests import markdup_model as md
from tests import test_host_bamsort as hs
from tests.bamsort_cases import H1, offsets
from tests.markdup_cases import bad_runs, cases, line, pair, records

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sim")
EINVAL = -22
REASONS = capi.BAMSORT_REASONS
_lib = None


def sim_lib():
    """tests/host_sim/libmarkdup_sim.so, built beside the other host-sim libraries and leaving them alone"""
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "libmarkdup_sim.so")
        src = os.path.join(HERE, "markdup_sim.cpp")
        deps = [src] + [os.path.join(capi.CSRC, f) for f in ("bam_dup_core.h", "bam_sort_core.h", "bam_core.h")] + [os.path.join(os.path.dirname(capi.HERE), "include", "moni_hip.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
        L = C.CDLL(so)
        L.markdupsim_run.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.markdupsim_resolve.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.markdupsim_setdup.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
        L.markdupsim_setdup.restype = None
        L.markdupsim_bits.argtypes = [C.c_uint32]
        L.markdupsim_bits.restype = C.c_uint32
        _lib = L
    return _lib


def sim_run(n_ref, recs, paired):
    """(rc, the run's entries as BAM_DUP_DTYPE, stats) of the replay; the buffers are exactly as large as the input says"""
    data = np.frombuffer(b"".join(recs), dtype=np.uint8)
    off = offsets(recs)
    ents, n_ent, st = np.zeros(max(len(recs), 1), capi.BAM_DUP_DTYPE), C.c_uint64(), np.zeros(3, np.uint64)
    rc = sim_lib().markdupsim_run(n_ref, data.ctypes.data if data.size else None, data.size, off.ctypes.data, len(recs), int(paired), ents.ctypes.data, C.byref(n_ent),
                                  st.ctypes.data)
    return rc, ents[:n_ent.value].copy(), dict(bad_records=int(st[0]), first_bad_record=int(st[1]), bad_reason=int(st[2]))


def sim_resolve(n_ref, dups, n_records):
    """(rc, [marks of run r], stats)"""
    allents = np.concatenate([np.ascontiguousarray(d, dtype=capi.BAM_DUP_DTYPE) for d in dups]) if len(dups) else np.zeros(0, capi.BAM_DUP_DTYPE)
    nd, nr = np.array([len(d) for d in dups], np.uint64), np.array(list(n_records), np.uint64)
    marks, st = np.full(max(int(nr.sum()), 1), 0xEE, np.uint8), np.zeros(6, np.uint64)
    rc = sim_lib().markdupsim_resolve(n_ref, allents.ctypes.data if allents.size else None, nd.ctypes.data, nr.ctypes.data, len(dups), marks.ctypes.data, st.ctypes.data)
    cuts = np.concatenate([[0], np.cumsum(nr)]).astype(np.int64)
    stats = dict(bad_entries=int(st[0]), first_bad_entry=int(st[1]), pairs=int(st[2]), dup_pairs=int(st[3]), fragments=int(st[4]), dup_fragments=int(st[5]))
    return rc, [marks[cuts[r]:cuts[r + 1]].copy() for r in range(len(dups))], stats


def sim_setdup(recs, marks) -> bytes:
    buf = np.frombuffer(b"".join(recs), dtype=np.uint8).copy()
    off, m = offsets(recs), np.ascontiguousarray(marks, dtype=np.uint8)
    if len(recs):
        sim_lib().markdupsim_setdup(buf.ctypes.data, buf.size, off.ctypes.data, len(recs), m.ctypes.data)
    return buf.tobytes()


def model_of(header, paired, runs):
    """per run: the records in input order, the model's entries, their packed form; then the model's marks by sorted place, and its counts"""
    n_ref = len(bam.references(header))
    recs = [records(header, lines) for lines in runs]
    ents = [md.entries(r, paired, n_ref) for r in recs]
    where = [md.sorted_places(r, n_ref) for r in recs]
    marked = md.resolve(ents)
    marks = [np.zeros(len(r), np.uint8) for r in recs]
    for r, i in marked:
        marks[r][where[r][i]] = 1
    return n_ref, recs, ents, [md.pack_entries(e, w) for e, w in zip(ents, where)], marks, marked


CASES = cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_replay_equals_the_model(case):
    _, header, paired, runs = case
    n_ref, recs, ents, packed, want_marks, marked = model_of(header, paired, runs)
    dups = []
    for r, rr in enumerate(recs):
        rc, d, st = sim_run(n_ref, rr, paired)
        assert rc == 0 and st == dict(bad_records=0, first_bad_record=0, bad_reason=0)
        assert d.tobytes() == packed[r], "run %d: the replay's entries differ from the model's" % r
        dups.append(d)
    rc, marks, st = sim_resolve(n_ref, dups, [len(r) for r in recs])
    assert rc == 0
    for r in range(len(recs)):
        assert marks[r].tolist() == want_marks[r].tolist(), "run %d" % r
    p, dp, f, df, m = md.counts(ents, marked)
    assert (st["pairs"], st["dup_pairs"], st["fragments"], st["dup_fragments"], 2 * st["dup_pairs"] + st["dup_fragments"]) == (p, dp, f, df, m)
    # the records that leave the marked sort of every run: the model's flags on the model's order
    for r, rr in enumerate(recs):
        srt = bsm.sort_list(n_ref, rr)
        rc, got, _, _, sents, _ = hs.sim_sort(header, sim_setdup(srt, marks[r]), offsets(srt))
        want = bsm.sort_list(n_ref, md.set_flags(rr, [i for run, i in marked if run == r]))
        assert rc == 0 and got == b"".join(want)
        assert [int(x) & 0xFFFF for x in sents["bin_flag"]] == [struct.unpack_from("<H", x, 18)[0] for x in want]


def test_case_list_is_the_issues():
    by = {c[0]: c for c in CASES}
    for n in (0, 1, 2, 63, 64, 65, 257):
        assert len(by["se_n%d" % n][3][0]) == n and len(by["pe_n%d" % n][3][0]) == 2 * n
    n_ref, recs, ents, _, _, marked = model_of(*by["clips"][1:])
    u5 = [(e >> 1 & (2 ** 33 - 1)) - 2 ** 31 for e, _, _, _, _ in ents[0]]
    assert min(u5) < 0 and max(u5) > 2 ** 31 - 1 and u5.count(100) == 4 and u5.count(149) == 3 and u5.count(-7) == 3
    assert {int.from_bytes(r[16:18], "little") for r in recs[0]} >= {0, 1, 2, 3}
    assert {int.from_bytes(r[20:24], "little") for r in model_of(*by["lengths"][1:])[1][0]} == {0, 1, 63, 64, 65, 300}
    q = model_of(*by["qualities"][1:])
    assert [s for _, _, s, _, _ in q[2][0]] == [32 * 15, 0, 15, 0, 15, 5 * 93] and b"\xff" * 64 in q[1][0][1]
    n_ref, recs, ents, _, _, marked = model_of(*by["pairs"][1:])
    kinds = [k for _, _, _, k, _ in ents[0]]
    assert kinds == [1, 1, 1, 1, 3, 1, 1, 1, 1, 1] and ents[0][3][:2] == ents[0][4][:2]          # FF: the same ends, other kinds
    assert any(k1 >> 34 != k2 >> 34 for k1, k2, _, k, _ in ents[0] if k) and any(k1 == k2 for k1, k2, _, k, _ in ents[0] if k)
    names = lambda run: {recs[run][i][36:36 + recs[run][i][12] - 1].decode() for r, i in marked if r == run}
    assert names(0) == {"p0", "p1", "p5", "p7"} and names(1) == {"f0"}
    assert [k for _, _, _, k, _ in ents[1]] == [1, 0, 0]          # p10, f0's read 1, f2's read 2; none of f1 and f3
    assert len(by["runs_2"][3]) == 2 and len(by["runs_7"][3]) == 7 + 1 and [] in by["runs_7"][3] and not any(by["all_runs_empty"][3])
    r = model_of(*by["random2000"][1:])
    assert sum(len(x) for x in r[1]) == 4000 and len({k for e in r[2] for k1, k2, _, kind, _ in e for k in ((k1, k2) if kind else (k1,))}) <= 50
    assert sim_lib().markdupsim_bits(1) == 35 and sim_lib().markdupsim_bits(0) == 34 and sim_lib().markdupsim_bits(300) == 43


def test_fragment_groups_by_hand():
    """g1 and g3 score 1100, g7 1050, g0 1000 at (10, forward): g1 stays.  g2 (1000) and g8 (1250) at (59, reverse): g8 stays."""
    _, recs, _, _, _, marked = model_of(*{c[0]: c for c in CASES}["fragments"][1:])
    assert {recs[r][i][36:38] for r, i in marked} == {b"g0", b"g3", b"g7", b"g2"}


BAD = bad_runs()


@pytest.mark.parametrize("case", BAD, ids=[b[0] for b in BAD])
def test_bad_records(case):
    _, paired, lines, reason, first, count = case
    recs = records(H1, lines)
    with pytest.raises(md.MarkdupError) as x:
        md.entries(recs, paired, 1)
    assert (REASONS[x.value.reason], x.value.index, x.value.count) == (reason, first, count)
    rc, d, st = sim_run(1, recs, paired)
    assert rc == EINVAL and d.size == 0 and st == dict(bad_records=count, first_bad_record=first, bad_reason=REASONS.index(reason))


def test_seq_is_checked_before_the_qualities():
    """l_seq larger than the record holds: SEQ at the lowest index, in a buffer that ends with the last record"""
    good = records(H1, [x for i in range(6) for x in pair("n%d" % i, 10 * i, 0, 10 * i + 200, 16)])
    for at in ((3,), (9, 3), (11,)):
        recs = list(good)
        for k in at:
            recs[k] = recs[k][:20] + struct.pack("<I", 51 if k == 11 else 10 ** 9) + recs[k][24:]
        for paired in (True, False):
            rc, d, st = sim_run(1, recs, paired)
            assert rc == EINVAL and d.size == 0 and st == dict(bad_records=len(at), first_bad_record=min(at), bad_reason=REASONS.index("SEQ"))
            with pytest.raises(md.MarkdupError) as x:
                md.entries(recs, paired, 1)
            assert (x.value.reason, x.value.index) == (md.SEQ, min(at))
    # a record the sort refuses is refused with the sort's reason, before any of this
    rc, _, st = sim_run(1, good[:3] + [good[3][:8] + struct.pack("<i", -2) + good[3][12:]] + good[4:], True)
    assert rc == EINVAL and REASONS[st["bad_reason"]] == "POS" and st["first_bad_record"] == 3


def test_idx_out_of_range_is_refused():
    ok = np.array([(5, 0, 1, 0, (0, md.NONE)), (5, 9, 1, 1, (1, 0))], dtype=capi.BAM_DUP_DTYPE)
    assert sim_resolve(1, [ok], [2])[0] == 0
    for entry in ((5, 0, 1, 0, (2, md.NONE)), (5, 9, 1, 1, (1, 2)), (5, 9, 1, 1, (1, md.NONE)), (5, 0, 1, 0, (1, 0)), (5, 9, 1, 2, (1, 0))):
        bad = np.array([ok[0], entry, ok[1], entry], dtype=capi.BAM_DUP_DTYPE)
        rc, marks, st = sim_resolve(1, [ok, bad], [2, 2])
        assert rc == EINVAL and (st["bad_entries"], st["first_bad_entry"]) == (2, 3) and all((m == 0xEE).all() for m in marks)
    rc, marks, _ = sim_resolve(1, [ok[:0], ok], [0, 2])          # the run of an entry is found behind an empty one
    assert rc == 0 and marks[1].tolist() == [1, 0]          # the fragment lies at an end of the pair


def test_sanitizer_program():
    """markdup_sim.cpp as a program of its own under AddressSanitizer and UBSan: the built-in cases in buffers sized exactly"""
    exe = os.path.join(HERE, "markdup_sim_asan")
    src = os.path.join(HERE, "markdup_sim.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DMARKDUP_SIM_MAIN", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True)
    assert r.returncode == 0 and b"0 case(s) failed" in r.stdout and b"FAILED" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
