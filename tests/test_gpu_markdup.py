"""Duplicate marking on the GPU: Ctx.bam_sorted_run_dup gives, byte for byte, the entries of the host replay of the same per-record code
(tests/test_host_markdup.py) on every input of that file, Ctx.bam_dup_resolve its marks, Ctx.bam_sort_marked(raw=True) the records and index
entries of the replay's flag pass and sort; the first four results of bam_sorted_run_dup are bam_sorted_run's; marks of None are bam_sort; bad
records and entries are refused with the replay's counts; none of it depends on the context; the context's other state is left alone.

MONI_BAMSORT_SEQ cannot be reached through the library: moni_bam_sorted_run_dup takes SAM text, and the encoder writes no record whose l_seq
exceeds it.  The check guards the kernel's loads; the replay holds it (tests/test_host_markdup.py)."""
import ctypes as C
import threading

import numpy as np
import pytest

from tests import bam_model as bam
from tests import bamsort_model as bsm
from tests import markdup_model as md
from tests import test_host_bamsort as hb
from tests import test_host_markdup as hm
from tests.bamsort_cases import H1, H2, offsets
from tests.markdup_cases import records
from tests.test_bam_model import SAMS, golden

pytestmark = pytest.mark.gpu

EINVAL = -22


@pytest.fixture(scope="module")
def rig(small_case):
    from moni_align_amd import capi
    idx = capi.Index(fi=small_case.fi, device=0)
    ctx = capi.Ctx(idx)
    yield capi, idx, ctx
    ctx.close()
    idx.close()


def check(ctx, header, paired, runs):
    """the three calls on one case against the replay; returns the marked, sorted records of every run"""
    n_ref = len(bam.references(header))
    ctx.bam_set_header(header)
    dups, n_rec, srt, out = [], [], [], []
    for lines in runs:
        recs = records(header, lines)
        rc, want, _ = hm.sim_run(n_ref, recs, paired)
        assert rc == 0
        rec, keys, offs, d, st = ctx.bam_sorted_run_dup(b"".join(lines), paired)
        assert d.tobytes() == want.tobytes(), "the kernels' entries differ from the host replay's"
        plain = ctx.bam_sorted_run(b"".join(lines))
        assert rec == plain[0] and np.array_equal(keys, plain[1]) and np.array_equal(offs, plain[2])
        assert (st["entries"], st["pairs"], st["fragments"]) == (len(want), int((want["kind"] != 0).sum()), int((want["kind"] == 0).sum()))
        assert (st["bad_records"], st["bad_is_record"], st["records"]) == (0, 0, len(recs)) and (not recs or (st["t_sig"] > 0 and st["t_entry"] > 0))
        dups.append(d); n_rec.append(len(recs)); srt.append((rec, offs))
    rc, want_marks, wst = hm.sim_resolve(n_ref, dups, n_rec)
    assert rc == 0
    marks, st = ctx.bam_dup_resolve(dups, n_rec)
    for r in range(len(runs)):
        assert marks[r].tobytes() == want_marks[r].tobytes(), "run %d: the kernels' marks differ from the host replay's" % r
    assert {k: st[k] for k in ("pairs", "dup_pairs", "fragments", "dup_fragments")} == {k: wst[k] for k in ("pairs", "dup_pairs", "fragments", "dup_fragments")}
    assert st["marked_records"] == sum(int(m.sum()) for m in marks) and st["entries"] == sum(len(d) for d in dups) and st["bad_entries"] == 0
    assert st["t_total"] >= 0 and (not st["entries"] or (st["t_sort"] > 0 and st["t_flag"] > 0))
    for r, (rec, offs) in enumerate(srt):
        recs = bsm.split_records(rec)
        rc, want, _, woff, wents, _ = hb.sim_sort(header, hm.sim_setdup(recs, marks[r]), offs)
        assert rc == 0
        raw, ents, _ = ctx.bam_sort_marked(rec, offs, marks[r], raw=True)
        assert raw == want and np.array_equal(ents, wents), "run %d: the marked sort differs from the host replay's" % r
        assert sum(1 for x in bsm.split_records(raw) if x[19] & 4) == int(marks[r].sum())
        a, b = ctx.bam_sort_marked(rec, offs, None, raw=True), ctx.bam_sort(rec, offs, raw=True)
        assert a[0] == b[0] == rec and np.array_equal(a[1], b[1])
        out.append(raw)
    return out


@pytest.mark.parametrize("case", hm.CASES, ids=[c[0] for c in hm.CASES])
def test_kernels_equal_host_replay(rig, case):
    _, header, paired, runs = case
    check(rig[2], header, paired, runs)


@pytest.mark.parametrize("name", SAMS)
def test_golden_sam(rig, name):
    """the golden SAM files: the run is moni_bam_sorted_run's, the entries the model's; the compressed marked sort is moni_bam_sort's blocks where no mark is set"""
    capi, _, ctx = rig
    header, lines = golden(name)
    paired = name.startswith("pe_")
    n_ref = len(bam.references(header))
    recs = bsm.split_records(bam.encode_records(header, lines))
    ctx.bam_set_header(header)
    rec, keys, offs, d, st = ctx.bam_sorted_run_dup(lines, paired)
    plain = ctx.bam_sorted_run(lines)
    assert rec == plain[0] and keys.tobytes() == plain[1].tobytes() and offs.tobytes() == plain[2].tobytes()
    assert d.tobytes() == md.pack_entries(md.entries(recs, paired, n_ref), md.sorted_places(recs, n_ref))
    marks, _ = ctx.bam_dup_resolve([d], [len(recs)])
    marked = md.resolve([md.entries(recs, paired, n_ref)])
    assert rec != b"" and bsm.split_records(ctx.bam_sort_marked(rec, offs, marks[0], raw=True)[0]) == bsm.sort_list(n_ref, md.set_flags(recs, [i for _, i in marked]))
    zero = np.zeros(len(recs), np.uint8)
    assert ctx.bam_sort_marked(rec, offs, zero, eof=True)[0] == ctx.bam_sort(rec, offs, eof=True)[0] == ctx.bam_sort_marked(rec, offs, None, eof=True)[0]


def test_empty(rig):
    capi, _, ctx = rig
    ctx.bam_set_header(H2)
    rec, keys, offs, d, st = ctx.bam_sorted_run_dup(b"", True)
    assert rec == b"" and keys.size == 0 and offs.tolist() == [0] and d.size == 0 and st["entries"] == 0
    for dups, n in (([], []), ([d, d], [0, 0]), ([d], [5])):
        marks, st = ctx.bam_dup_resolve(dups, n)
        assert [m.tolist() for m in marks] == [[0] * k for k in n] and st["marked_records"] == 0
    out, ents, _ = ctx.bam_sort_marked(b"", np.zeros(1, np.uint64), np.zeros(0, np.uint8), raw=True)
    assert out == b"" and ents.size == 0


@pytest.mark.parametrize("case", hm.BAD, ids=[b[0] for b in hm.BAD])
def test_bad_records(rig, case):
    capi, _, ctx = rig
    _, paired, lines, reason, first, count = case
    want = hm.sim_run(1, records(H1, lines), paired)
    assert want[0] == EINVAL
    ctx.bam_set_header(H1)
    with pytest.raises(capi.BamBadRecord) as e:
        ctx.bam_sorted_run_dup(b"".join(lines), paired)
    st = e.value.stats
    assert (st["bad_records"], st["first_bad_record"], st["bad_reason"]) == (want[2]["bad_records"], want[2]["first_bad_record"], want[2]["bad_reason"]) == \
        (count, first, capi.BAMSORT_REASONS.index(reason))
    assert st["bad_is_record"] == 1 and st["entries"] == 0
    # a bad line is still the encoder's
    with pytest.raises(capi.BamBadLine):
        ctx.bam_sorted_run_dup(b"r\t0\tchr1\n", paired)
    ok = ctx.bam_sorted_run_dup(b"".join(lines), False) if reason == "MATE" else None          # single-end: the same lines pass
    assert ok is None or len(ok[3]) == len(lines)


def test_bad_entries(rig):
    capi, _, ctx = rig
    ctx.bam_set_header(H1)
    ok = np.array([(5, 0, 1, 0, (0, md.NONE)), (5, 9, 1, 1, (1, 0))], dtype=capi.BAM_DUP_DTYPE)
    assert [m.tolist() for m in ctx.bam_dup_resolve([ok[:0], ok], [0, 2])[0]] == [[], [1, 0]]
    for entry in ((5, 0, 1, 0, (2, md.NONE)), (5, 9, 1, 1, (1, 2)), (5, 9, 1, 1, (1, md.NONE)), (5, 0, 1, 0, (1, 0)), (5, 9, 1, 2, (1, 0))):
        bad = np.array([ok[0], entry, ok[1], entry], dtype=capi.BAM_DUP_DTYPE)
        want = hm.sim_resolve(1, [ok, bad], [2, 2])
        assert want[0] == EINVAL
        L = capi.lib()
        marks = [np.full(2, 0xEE, np.uint8), np.full(2, 0xEE, np.uint8)]
        dp = (C.c_void_p * 2)(ok.ctypes.data, bad.ctypes.data)
        mp = (C.c_void_p * 2)(marks[0].ctypes.data, marks[1].ctypes.data)
        nd, nr, st = np.array([2, 4], np.uint64), np.array([2, 2], np.uint64), capi.BamDupStatsC()
        assert L.moni_bam_dup_resolve(ctx._h, dp, nd.ctypes.data, nr.ctypes.data, 2, mp, C.byref(st)) == EINVAL
        assert (st.bad_entries, st.first_bad_entry) == (want[2]["bad_entries"], want[2]["first_bad_entry"]) == (2, 3)
        assert all((m == 0xEE).all() for m in marks), "a refused call wrote marks"
        with pytest.raises(capi.BamBadEntry):
            ctx.bam_dup_resolve([ok, bad], [2, 2])


def test_errors(rig):
    capi, idx, ctx = rig
    L = capi.lib()
    by = {c[0]: c for c in hm.CASES}
    lines = b"".join(by["pe_n63"][3][0])
    fresh = capi.Ctx(idx)          # before a header is set
    try:
        with pytest.raises(RuntimeError, match="-22"):
            fresh.bam_sorted_run_dup(lines, True)
        with pytest.raises(RuntimeError, match="-22"):
            fresh.bam_dup_resolve([], [])
        with pytest.raises(RuntimeError, match="-22"):
            fresh.bam_sort_marked(b"", np.zeros(1, np.uint64), None, raw=True)
    finally:
        fresh.close()
    ctx.bam_set_header(H2)
    with pytest.raises(RuntimeError, match="-22"):
        ctx.bam_sorted_run_dup(lines, 2)
    rec, rl, keys, offs, n, dups, nd, st = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64(7), capi.BamRunDupStatsC()
    args = [ctx._h, lines, len(lines), 1, C.byref(rec), C.byref(rl), C.byref(keys), C.byref(offs), C.byref(n), C.byref(dups), C.byref(nd), C.byref(st)]
    assert L.moni_bam_sorted_run_dup(*args) == 0 and nd.value == 63 and n.value == 126
    for k in (0, 4, 5, 6, 7, 8, 9, 10):
        a = list(args)
        a[k] = None
        assert L.moni_bam_sorted_run_dup(*a) == EINVAL, k
    a = list(args)
    a[11] = None          # the stats may be NULL
    assert L.moni_bam_sorted_run_dup(*a) == 0
    d = np.zeros(1, capi.BAM_DUP_DTYPE)
    one = (C.c_void_p * 1)(d.ctypes.data)
    m = np.zeros(1, np.uint8)
    mp = (C.c_void_p * 1)(m.ctypes.data)
    cnt = np.ones(1, np.uint64)
    assert L.moni_bam_dup_resolve(None, one, cnt.ctypes.data, cnt.ctypes.data, 1, mp, None) == EINVAL
    assert L.moni_bam_dup_resolve(ctx._h, None, cnt.ctypes.data, cnt.ctypes.data, 1, mp, None) == EINVAL
    assert L.moni_bam_dup_resolve(ctx._h, one, None, cnt.ctypes.data, 1, mp, None) == EINVAL
    assert L.moni_bam_dup_resolve(ctx._h, one, cnt.ctypes.data, None, 1, mp, None) == EINVAL
    assert L.moni_bam_dup_resolve(ctx._h, one, cnt.ctypes.data, cnt.ctypes.data, 1, None, None) == EINVAL
    d["idx"][0] = (0, md.NONE)
    assert L.moni_bam_dup_resolve(ctx._h, one, cnt.ctypes.data, cnt.ctypes.data, 1, mp, None) == 0 and m[0] == 0
    assert L.moni_bam_dup_resolve(ctx._h, None, None, None, 0, None, None) == 0


def test_two_contexts_two_threads(rig):
    capi, idx, _ = rig
    by = {c[0]: c for c in hm.CASES}
    inputs = [by["random2000"], by["runs_7"]]
    got, want, errs = [None, None], [None, None], []

    def work(k):
        try:
            ctx = capi.Ctx(idx)
            try:
                _, h, paired, runs = inputs[k]
                for _ in range(2):
                    got[k] = check(ctx, h, paired, runs)
            finally:
                ctx.close()
        except BaseException as e:          # noqa: B036 - handed to the main thread
            errs.append(e)

    ts = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for k in range(2):
        _, h, paired, runs = inputs[k]
        n_ref, recs, _, _, _, marked = hm.model_of(h, paired, runs)
        want[k] = [b"".join(bsm.sort_list(n_ref, md.set_flags(rr, [i for run, i in marked if run == r]))) for r, rr in enumerate(recs)]
    assert got == want


def test_align_state_is_left_alone(rig, small_case):
    """the SAM text of an align_batch is marked; the batch, the counters, the kernel times and a pending fetch stay"""
    capi, idx, ctx = rig
    synth = small_case.synth
    reads = synth.make_reads(small_case.pg, 300, 150, seed=5)
    reads = np.concatenate([reads, reads[:60]])          # sixty reads come twice
    offs = np.arange(0, (len(reads) + 1) * 150, 150, dtype=np.uint64)
    names, noff = synth.make_names(len(reads))
    quals = np.full(reads.size, ord("I"), dtype=np.uint8)
    quals[300 * 150:] = ord("5")
    sam, st = ctx.align_batch(reads.reshape(-1), offs, names, noff, quals, host_threads=2, stream=True)
    assert st["aligned"] > 0
    header = ctx.sam_header()
    ctx.bam_set_header(header)
    n_ref = len(bam.references(header))

    def state():
        ms = {}
        for which in range(7):
            try:
                ms[which] = ctx.kernel_ms(which)
            except RuntimeError:          # that stage did not run
                pass
        return ms, ctx.counters().tolist()

    before = state()
    assert before[0]
    rec, keys, roff, d, _ = ctx.bam_sorted_run_dup(sam, False)
    recs = bsm.split_records(bam.encode_records(header, sam))
    marked = md.resolve([md.entries(recs, False, n_ref)])
    mapped_copies = sum(1 for i in range(60) if not recs[i][18] & 4 and not recs[300 + i][18] & 4)
    assert mapped_copies > 30 and len(marked) >= mapped_copies
    marks, _ = ctx.bam_dup_resolve([d], [len(recs)])
    z, ents, _ = ctx.bam_sort_marked(rec, roff, marks[0], eof=True)
    from tests import bgzf_model as bm
    assert b"".join(b for b, _ in bm.walk(z)) == b"".join(bsm.sort_list(n_ref, md.set_flags(recs, [i for _, i in marked])))
    assert state() == before
    sam2, st2 = ctx.align_batch(reads.reshape(-1), offs, names, noff, quals, host_threads=2, stream=True)
    assert sam2 == sam and st2["aligned"] == st["aligned"]
    ctx.upload(reads.reshape(-1), offs)
    ctx.screen_run()
    ctx.bam_sorted_run_dup(sam, False)
    ctx.bam_dup_resolve([d], [len(recs)])
    ctx.bam_sort_marked(rec, roff, marks[0])
    res = ctx.screen_fetch()
    assert len(res) == len(reads) and np.array_equal(res, ctx.screen_batch(reads.reshape(-1), offs))
