"""Per-sequence occurrence counts on the GPU: count_kernel, seqcount_plan_kernel, the scan, seqcount_walk_kernel and seqcount_finish_kernel through
the C ABI (Ctx.seqcount_batch / seqcount_run + seqcount_fetch + seqcount_sizes) against brute force that shares no code with the library - all
start positions of the pattern by direct search of the text, binned with numpy.searchsorted on the sequence starts.  A parity check: no
tolerance."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import locate_model as lm
from tests import seqcount_model as sm

pytestmark = pytest.mark.gpu


class Rig:
    def __init__(self, fi, without_lcp=False):
        from moni_align_amd import capi
        self.fi = fi
        self.text = fi.text.tobytes()
        self.idx = capi.Index(fi=fi, device=0, without_lcp=without_lcp)
        self.ctx = capi.Ctx(self.idx)

    def check(self, pats, strands, max_walk=1 << 20, ctx=None):
        ctx = ctx or self.ctx
        res, counts = ctx.seqcount_batch(*lm.ragged(pats), strands=strands, max_walk=max_walk)
        sm.check_against_brute(self.text, pats, res, counts, strands, max_walk, self.fi.seq_starts)
        invariants(res, counts, ctx.counters())
        return res, counts

    def close(self):
        self.ctx.close()
        self.idx.close()


def invariants(res, counts, c):
    """row sums against count, n_seqs against the table, the phi-step counter against sum (count - n_segs) over the walked tasks"""
    w = res["walked"] != 0
    assert np.array_equal(counts.sum(axis=1)[w], res["count"][w]) and not counts[~w].any()
    assert np.array_equal((counts != 0).sum(axis=1), res["n_seqs"])
    assert not res["n_segs"][~w].any() and np.array_equal(res["n_segs"] > 0, w & (res["count"] > 0))
    assert int(c[2]) == int((res["count"][w].astype(np.int64) - res["n_segs"][w]).sum())


@pytest.fixture(scope="module")
def case():
    return lm.planted_case()


@pytest.fixture(scope="module")
def rig(case):
    r = Rig(case[0])
    yield r
    r.close()


@pytest.mark.parametrize("strands", [1, 2])
def test_patterns_against_brute_force(rig, case, strands):
    pats = case[2] + [b"A", b"C", b"G", b"T", b"AC"]
    res, counts = rig.check(pats, strands)
    c = rig.ctx.counters()
    assert int(c[0]) > 0 and int(c[3]) > 0 and int(c[2]) > 0
    unit = res[19 * strands]
    assert int(unit["count"]) >= 9 and int(unit["matched"]) == 40 and int(unit["n_seqs"]) == 3 and int(unit["walked"]) == 1
    assert int(res["n_segs"].max()) >= 100 and int((res["n_segs"] == 1).sum()) > 0 and res["walked"].all()
    for k, want in ((24, 0), (25, 0), (26, 0), (27, 19), (28, 39), (29, 39), (30, 19)):          # empty; an absent byte last, middle, first; dead at the last and a middle step
        assert int(res["count"][k * strands]) == 0 and int(res["matched"][k * strands]) == want and int(res["n_segs"][k * strands]) == 0, k
    assert rig.ctx.kernel_ms(0) > 0 and rig.ctx.kernel_ms(3) > 0 and rig.ctx.kernel_ms(6) >= rig.ctx.kernel_ms(3)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_batch_sizes(rig, case, n):
    """block and wave tails of the task kernels (the patterns in turn, from another start for every size)"""
    pats = case[2]
    batch = [pats[(7 * n + k) % len(pats)] for k in range(n)]
    rig.check(batch, 2)
    rig.check(batch, 1)


def test_max_walk(rig, case):
    pats = case[2]
    full, full_counts = rig.check(pats, 2, 0)                    # no limit
    assert full["walked"].all()
    res, counts = rig.check(pats, 2, 8)
    unit = res[19 * 2]
    assert int(unit["count"]) >= 9 and int(unit["walked"]) == 0 and int(unit["n_seqs"]) == 0 and int(unit["n_segs"]) == 0 and not counts[19 * 2].any()
    for k in ("count", "sa_lo", "matched"):                      # exact whether or not the task was walked
        assert np.array_equal(res[k], full[k]), k
    w = res["walked"] != 0
    assert np.array_equal(w, full["count"] <= 8) and 0 < int(w.sum()) < len(w)
    assert np.array_equal(counts[w], full_counts[w]) and np.array_equal(res["n_seqs"][w], full["n_seqs"][w]) and np.array_equal(res["n_segs"][w], full["n_segs"][w])
    deflt, _ = rig.check(pats, 2)
    assert np.array_equal(deflt, full)


def test_run_fetch_sizes(rig, case):
    from moni_align_amd import capi
    pats = case[2]
    big, small = pats[:40], pats[40:] + [b""]
    cx = capi.Ctx(rig.idx)
    try:
        p = cx._seqcount_params(1, 0)
        assert cx._L.moni_seqcount_fetch(cx._h, None, None) == -22 and cx._L.moni_seqcount_sizes(cx._h, None, None) == -22          # nothing was run yet
        assert cx._L.moni_seqcount_run(cx._h, ctypes.byref(p)) == -22                                                               # no batch is resident
        cx.upload(*lm.ragged(big))
        cx.swap(0)                                   # big parked
        cx.upload(*lm.ragged(small))
        cx.swap(0)                                   # big resident again, small parked
        cx.seqcount_run(strands=2)
        assert cx.seqcount_sizes() == (2 * len(big), len(rig.fi.seq_starts) - 1)
        res, counts = cx.seqcount_fetch()
        sm.check_against_brute(rig.text, big, res, counts, 2, 1 << 20, rig.fi.seq_starts)
        invariants(res, counts, cx.counters())
        only, none = cx.seqcount_fetch(want_counts=False)
        assert np.array_equal(only, res) and none is None
        cx.swap(0)                                   # small resident: the last run's results are gone with its batch
        with pytest.raises(RuntimeError):
            cx.seqcount_fetch()
        cx.seqcount_run(strands=1, max_walk=8)
        res, counts = cx.seqcount_fetch()
        sm.check_against_brute(rig.text, small, res, counts, 1, 8, rig.fi.seq_starts)
        cx.upload(*lm.ragged(big))                   # fetch after moni_reads_upload
        assert cx._L.moni_seqcount_fetch(cx._h, None, None) == -22 and cx._L.moni_seqcount_sizes(cx._h, None, None) == -22
        cx.seqcount_run(strands=1)
        cx.locate_batch(*lm.ragged(small), strands=1, max_occ=2)          # ... and after another query's *_batch call
        assert cx._L.moni_seqcount_fetch(cx._h, None, None) == -22
    finally:
        cx.close()


def test_invalid_parameters(rig, case):
    from moni_align_amd import capi
    L = rig.ctx._L
    b, keep = rig.ctx._batch(*lm.ragged(case[2][:3]))
    res = np.zeros(6, dtype=capi.SEQCOUNT_RES_DTYPE)
    rig.ctx.upload(*lm.ragged(case[2][:3]))
    for strands, reserved in ((0, 0), (3, 0), (1, 1), (2, 7)):
        p = capi.SeqcountParamsC(strands, reserved, 0)
        assert L.moni_seqcount_run(rig.ctx._h, ctypes.byref(p)) == -22
        assert L.moni_seqcount_batch(rig.ctx._h, ctypes.byref(b), ctypes.byref(p), res.ctypes.data, None) == -22
    assert L.moni_seqcount_run(rig.ctx._h, None) == -22
    p = capi.SeqcountParamsC(2, 0, 0)
    assert L.moni_seqcount_batch(rig.ctx._h, ctypes.byref(b), ctypes.byref(p), res.ctypes.data, None) == 0          # counts may be NULL
    assert int(res["count"].sum()) > 0


def test_empty_batch_and_empty_patterns(rig):
    res, counts = rig.ctx.seqcount_batch(np.zeros(0, np.uint8), np.zeros(1, np.uint64), strands=2)
    assert len(res) == 0 and counts.shape[0] == 0
    res, counts = rig.check([b"", b""], 2)
    assert not res["count"].any() and not res["matched"].any() and not counts.any() and res["walked"].all()


def test_index_without_lcp_samples(case):
    r = Rig(case[0], without_lcp=True)
    try:
        r.check(case[2], 2)
    finally:
        r.close()


def test_long_runs_and_a_skewed_batch():
    """W: 6000 occurrences behind one BWT run of 4095 or more (one segment of 6000 steps); substrings of it; then one such task among 128 with at
    most 2 occurrences: a segment count that is no multiple of 64, and segments of very different length in one wave"""
    from tests.test_host_sim import long_run_case
    fi, reads = long_run_case()
    r = Rig(fi)
    try:
        text = r.text
        W = text[13:53]
        res, counts = r.check([W, W[:20], W[5:], b"C" + W, text[12:53], b"NNNN", b"ANNNN"], 2)
        assert int(res["count"][0]) == 6000 and int(res["n_segs"][0]) == 1 and int(counts[0, 0]) == 6000
        rare = [text[a:a + 70] for a in range(7, 7 + 128 * 67, 67)]
        skew = rare[:50] + [W] + rare[50:]
        res, counts = r.check(skew, 1)
        others = np.delete(res["count"], 50)
        assert int(res["count"][50]) == 6000 and int(others.max()) <= 2 and int(others.min()) >= 1
        assert int(res["n_segs"].sum()) % 64 != 0
        res, counts = r.check([b"C", b"N", W], 1, 0)             # a letter: an interval over a hundred thousand positions and thousands of runs
        assert int(res["count"][0]) >= 100000 and int(res["n_segs"][0]) >= 1000 and int(res["count"][1]) == 48
    finally:
        r.close()


def test_two_contexts_from_two_threads(rig, case):
    from moni_align_amd import capi
    pats = case[2]
    halves = [pats[0::2], pats[1::2]]
    ctxs = [capi.Ctx(rig.idx), capi.Ctx(rig.idx)]
    try:
        def work(k):
            return [ctxs[k].seqcount_batch(*lm.ragged(halves[k]), strands=2, max_walk=0 if k else 8) for _ in range(4)]
        with ThreadPoolExecutor(2) as ex:
            outs = list(ex.map(work, (0, 1)))
        for k in (0, 1):
            sm.check_against_brute(rig.text, halves[k], *outs[k][0], 2, 0 if k else 8, rig.fi.seq_starts)
            for o in outs[k][1:]:
                assert all(np.array_equal(a, b) for a, b in zip(o, outs[k][0]))
    finally:
        for c in ctxs:
            c.close()


def test_agrees_with_locate_binned_on_the_host(rig, case):
    """the route a caller had before: every occurrence listed by moni_locate, binned with numpy.bincount - on the same context"""
    pats = case[2] + [b"A", b"AC"]
    n_seq = len(rig.fi.seq_starts) - 1
    lres, pos, sq, so = rig.ctx.locate_batch(*lm.ragged(pats), strands=2, max_occ=1 << 20)
    res, counts = rig.ctx.seqcount_batch(*lm.ragged(pats), strands=2)
    assert np.array_equal(lres["count"], res["count"]) and np.array_equal(lres["sa_lo"], res["sa_lo"]) and np.array_equal(lres["matched"], res["matched"])
    for t, r in enumerate(lres):
        a, k = int(r["occ_off"]), int(r["n_occ"])
        assert k == int(r["count"])
        assert np.array_equal(np.bincount(sq[a:a + k], minlength=n_seq).astype(np.uint64), counts[t]), t
