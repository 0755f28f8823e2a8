"""Reference loci on the GPU: count_kernel, seqcount_plan_kernel, loci_plan_kernel, the scans, loci_walk_kernel, the radix sort and the fold through
the C ABI (Ctx.loci_batch / loci_run + loci_fetch + loci_sizes) against brute force that shares no code with the library - all start positions of the
pattern by direct search of the text, the haplotype-to-reference map walked from the pangenome's variant lists, a Counter.  A parity check: no
tolerance."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import locate_model as lm
from tests import loci_model as lo

pytestmark = pytest.mark.gpu

ENOMEM, EINVAL = -12, -22


class Rig:
    def __init__(self, fi, keymap=None, without_lcp=False):
        from moni_align_amd import capi
        self.fi = fi
        self.text = fi.text.tobytes()
        self.keymap = keymap
        self.idx = capi.Index(fi=fi, device=0, without_lcp=without_lcp)
        self.ctx = capi.Ctx(self.idx)

    def check(self, pats, strands, lift=1, max_walk=1 << 20, ctx=None):
        ctx = ctx or self.ctx
        out = ctx.loci_batch(*lm.ragged(pats), strands=strands, lift=lift, max_walk=max_walk)
        lo.check_against_brute(self.text, pats, out, strands, max_walk, self.fi.seq_starts, self.keymap if lift else None)
        invariants(out, ctx.counters())
        return out

    def close(self):
        self.ctx.close()
        self.idx.close()


def invariants(out, c):
    """supports against count, the order inside a task, the phi-step counter against sum (count - n_segs) over the walked tasks"""
    res, lpos, lseq, lseq_off, support = out
    w = res["walked"] != 0
    assert not res["n_segs"][~w].any() and not res["n_loci"][~w].any() and np.array_equal(res["n_segs"] > 0, w & (res["count"] > 0))
    assert int(res["n_loci"].sum()) == len(lpos) and int(support.sum()) == int(res["count"][w].sum()) and (support > 0).all()
    for r in res:
        a, k = int(r["loci_off"]), int(r["n_loci"])
        assert (np.diff(lpos[a:a + k].astype(np.int64)) > 0).all() and (not k or int(support[a:a + k].sum()) == int(r["count"]))
    assert int(c[2]) == int((res["count"][w].astype(np.int64) - res["n_segs"][w]).sum())


@pytest.fixture(scope="module")
def case():
    pg, fi, text, pats = lo.lifted_case()
    return pg, fi, text, pats, lo.text_to_ref(pg)


@pytest.fixture(scope="module")
def rig(case):
    r = Rig(case[1], case[4])
    yield r
    r.close()


@pytest.mark.parametrize("strands,lift", [(1, 1), (2, 1), (1, 0), (2, 0)])
def test_patterns_against_brute_force(rig, case, strands, lift):
    pg, fi, text, pats, keymap = case
    res, lpos, lseq, lseq_off, support = rig.check(pats, strands, lift)
    c = rig.ctx.counters()
    assert int(c[0]) > 0 and int(c[2]) > 0 and res["walked"].all()
    assert int(res["n_segs"].max()) >= 200 and int((res["n_segs"] == 1).sum()) > 0
    a = res[0]                                                   # the pattern A
    assert int(a["count"]) == 9125 and int(a["n_loci"]) == (1527 if lift else 9125)
    if lift:
        assert int(support.max()) == 8 > len(pg.seqs)            # an insertion folded: more support than there are sequences
        r32 = res[2 * strands]
        assert int(r32["n_loci"]) == 1 and (int(lpos[int(r32["loci_off"])]), int(support[int(r32["loci_off"])])) == (1000, len(pg.seqs))
        r20 = res[3 * strands]                                   # starts inside haplotype 1's insertion in front of reference base 2784
        assert 2784 in lpos[int(r20["loci_off"]):int(r20["loci_off"]) + int(r20["n_loci"])].tolist()
        assert (lseq == 0).all() and np.array_equal(lseq_off, lpos)          # every haplotype lifts onto sequence 0, which starts the text
    else:
        assert (support == 1).all()
    assert rig.ctx.kernel_ms(0) > 0 and rig.ctx.kernel_ms(3) > 0 and rig.ctx.kernel_ms(4) > 0 and rig.ctx.kernel_ms(6) >= rig.ctx.kernel_ms(3)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_batch_sizes(rig, case, n):
    """block and wave tails of the task kernels (the patterns in turn, from another start for every size; A is pattern 0)"""
    pats = case[3]
    batch = [pats[(7 * n + k) % len(pats)] for k in range(n)]
    rig.check(batch, 2, 1)
    rig.check(batch, 1, 0)


def test_a_alone_and_among_rare_patterns(rig, case):
    """one task of thousands of occurrences and hundreds of segments, alone and in the middle of 128 tasks of a handful: segments of very different
    length in one wave, a task index in the sort key's high bits"""
    pg, fi, text, pats, keymap = case
    ref = pg.seqs[0].tobytes()
    res, lpos, lseq, lseq_off, support = rig.check([b"A"], 1, 1)
    assert int(res["n_loci"][0]) == 1527 and int(support.max()) == 8
    rare = [ref[a:a + 30] for a in range(11, 11 + 128 * 43, 43)]
    skew = rare[:50] + [b"A"] + rare[50:]
    for lift in (1, 0):
        res, lpos, lseq, lseq_off, support = rig.check(skew, 1, lift)
        others = np.delete(res["count"], 50)
        assert int(res["count"][50]) == 9125 and int(others.max()) <= 12 and int(others.min()) >= 1


def test_max_walk(rig, case):
    pats = case[3]
    full = rig.check(pats, 2, 1, 0)                              # no limit
    assert full[0]["walked"].all()
    out = rig.check(pats, 2, 1, 8)
    res = out[0]
    assert int(res["count"][0]) == 9125 and int(res["walked"][0]) == 0 and int(res["n_loci"][0]) == 0
    for k in ("count", "sa_lo", "matched"):                      # exact whether or not the task was walked
        assert np.array_equal(res[k], full[0][k]), k
    w = res["walked"] != 0
    assert np.array_equal(w, full[0]["count"] <= 8) and 0 < int(w.sum()) < len(w)
    assert np.array_equal(res["n_loci"][w], full[0]["n_loci"][w]) and np.array_equal(res["n_segs"][w], full[0]["n_segs"][w])
    deflt = rig.check(pats, 2, 1)
    assert all(np.array_equal(a, b) for a, b in zip(deflt, full))


def test_max_total(rig, case):
    """a walked total over max_total: MONI_ENOMEM before anything is written, and the context goes on"""
    from moni_align_amd import capi
    pats = case[3]
    cx = capi.Ctx(rig.idx)
    try:
        cx.upload(*lm.ragged(pats))
        good = cx._loci_params(2, 1, 1 << 20, None)
        assert cx._L.moni_loci_run(cx._h, ctypes.byref(good)) == 0
        res = cx.loci_fetch()[0]
        total = int(res["count"][res["walked"] != 0].sum())
        small = cx._loci_params(2, 1, 1 << 20, total - 1)
        assert cx._L.moni_loci_run(cx._h, ctypes.byref(small)) == ENOMEM
        assert cx._L.moni_loci_sizes(cx._h, None, None) == EINVAL          # the failed run left no result
        exact = cx._loci_params(2, 1, 1 << 20, total)
        assert cx._L.moni_loci_run(cx._h, ctypes.byref(exact)) == 0
        out = cx.loci_fetch()
        lo.check_against_brute(rig.text, pats, out, 2, 1 << 20, rig.fi.seq_starts, rig.keymap)
        tot8 = int(res["count"][res["count"] <= 8].sum())       # the limit counts walked tasks alone
        assert 0 < tot8 < total
        assert cx._L.moni_loci_run(cx._h, ctypes.byref(cx._loci_params(2, 1, 8, tot8))) == 0
        assert cx._L.moni_loci_run(cx._h, ctypes.byref(cx._loci_params(2, 1, 8, tot8 - 1))) == ENOMEM
        out = cx.loci_batch(*lm.ragged(pats), strands=2, max_total=0)          # no limit
        lo.check_against_brute(rig.text, pats, out, 2, 1 << 20, rig.fi.seq_starts, rig.keymap)
    finally:
        cx.close()


def test_run_fetch_sizes(rig, case):
    from moni_align_amd import capi
    pats = case[3]
    big, small = pats[:12], pats[12:] + [b""]
    cx = capi.Ctx(rig.idx)
    try:
        p = cx._loci_params(1, 1, 0, None)
        assert cx._L.moni_loci_fetch(cx._h, None, None, None, None, None) == EINVAL and cx._L.moni_loci_sizes(cx._h, None, None) == EINVAL          # nothing was run yet
        assert cx._L.moni_loci_run(cx._h, ctypes.byref(p)) == EINVAL                                                                                # no batch is resident
        cx.upload(*lm.ragged(big))
        cx.swap(0)                                   # big parked
        cx.upload(*lm.ragged(small))
        cx.swap(0)                                   # big resident again, small parked
        cx.loci_run(strands=2)
        out = cx.loci_fetch()
        assert cx.loci_sizes() == (2 * len(big), len(out[1]))
        lo.check_against_brute(rig.text, big, out, 2, 1 << 20, rig.fi.seq_starts, rig.keymap)
        invariants(out, cx.counters())
        only = cx.loci_fetch(want_loci=False)
        assert np.array_equal(only[0], out[0]) and len(only[1]) == 0
        cx.seqcount_run(strands=2)                   # another query on the same batch: the loci stay fetchable, and so do its results
        again = cx.loci_fetch()
        assert all(np.array_equal(a, b) for a, b in zip(again, out))
        cx.swap(0)                                   # small resident: the last run's results are gone with its batch
        with pytest.raises(RuntimeError):
            cx.loci_fetch()
        cx.loci_run(strands=1, lift=0, max_walk=8)
        lo.check_against_brute(rig.text, small, cx.loci_fetch(), 1, 8, rig.fi.seq_starts, None)
        cx.upload(*lm.ragged(big))                   # fetch after moni_reads_upload
        assert cx._L.moni_loci_fetch(cx._h, None, None, None, None, None) == EINVAL and cx._L.moni_loci_sizes(cx._h, None, None) == EINVAL
        cx.loci_run(strands=1)
        cx.locate_batch(*lm.ragged(small), strands=1, max_occ=2)          # ... and after another query's *_batch call
        assert cx._L.moni_loci_fetch(cx._h, None, None, None, None, None) == EINVAL
    finally:
        cx.close()


def test_invalid_parameters(rig, case):
    from moni_align_amd import capi
    L = rig.ctx._L
    pats = case[3][:3]
    b, keep = rig.ctx._batch(*lm.ragged(pats))
    res = np.zeros(6, dtype=capi.LOCI_RES_DTYPE)
    rig.ctx.upload(*lm.ragged(pats))
    u2 = ctypes.c_uint64 * 2
    for strands, lift, r0, r1 in ((0, 1, 0, 0), (3, 1, 0, 0), (1, 2, 0, 0), (1, 1, 1, 0), (2, 0, 0, 7)):
        p = capi.LociParamsC(strands, lift, 0, 0, u2(r0, r1))
        assert L.moni_loci_run(rig.ctx._h, ctypes.byref(p)) == EINVAL
        assert L.moni_loci_batch(rig.ctx._h, ctypes.byref(b), ctypes.byref(p), res.ctypes.data, None, None, None, None, None) == EINVAL
    assert L.moni_loci_run(rig.ctx._h, None) == EINVAL
    p = capi.LociParamsC(2, 1, 0, 0, u2(0, 0))
    assert L.moni_loci_batch(rig.ctx._h, ctypes.byref(b), ctypes.byref(p), res.ctypes.data, None, None, None, None, None) == 0          # the arrays may be NULL
    assert int(res["count"].sum()) > 0 and int(res["n_loci"].sum()) > 0


def test_empty_batch_and_empty_patterns(rig):
    out = rig.ctx.loci_batch(np.zeros(0, np.uint8), np.zeros(1, np.uint64), strands=2)
    assert all(len(a) == 0 for a in out)
    out = rig.check([b"", b""], 2)
    assert not out[0]["count"].any() and not out[0]["matched"].any() and not out[0]["n_loci"].any() and out[0]["walked"].all() and len(out[1]) == 0


def test_fasta_built_index_and_index_without_lcp_samples():
    """null lifts: lift = 1 gives the positions themselves; the same index without LCP samples"""
    pg, fi, text, pats = lo.lifted_case(lifted=False)
    for without_lcp in (False, True):
        r = Rig(fi, None, without_lcp=without_lcp)
        try:
            a = r.check(pats, 2, 1)
            b = r.check(pats, 2, 0)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)) and (a[4] == 1).all()
        finally:
            r.close()


def test_planted_case_without_lcp_samples():
    """three unrelated sequences with N runs (the general path of the search) and separator bytes in patterns, on an index without LCP samples"""
    fi, text, pats = lm.planted_case()
    pats = [p for p in pats if all(c > 5 for c in p)] + [b"A", b"N"]
    r = Rig(fi, None, without_lcp=True)
    try:
        out = r.check(pats, 2, 1)
        assert int(r.ctx.counters()[3]) > 0 and (out[4] == 1).all()
    finally:
        r.close()


def test_long_runs():
    """W: 6000 occurrences behind one BWT run of 4095 or more (one segment of 6000 slots); a letter whose interval spans thousands of runs"""
    from tests.test_host_sim import long_run_case
    fi, reads = long_run_case()
    r = Rig(fi)
    try:
        text = r.text
        W = text[13:53]
        out = r.check([W, W[:20], W[5:], b"C" + W, text[12:53], b"NNNN", b"ANNNN"], 2)
        assert int(out[0]["count"][0]) == 6000 and int(out[0]["n_segs"][0]) == 1 and int(out[0]["n_loci"][0]) == 6000
        res, lpos, lseq, lseq_off, support = r.ctx.loci_batch(*lm.ragged([b"C", W]), strands=1, lift=0, max_walk=0)
        invariants((res, lpos, lseq, lseq_off, support), r.ctx.counters())
        assert int(res["count"][0]) >= 100000 and int(res["n_segs"][0]) >= 1000
        assert np.array_equal(lpos[:int(res["n_loci"][0])], np.nonzero(np.frombuffer(text, np.uint8) == ord("C"))[0].astype(np.uint64))
    finally:
        r.close()


def test_two_contexts_from_two_threads(rig, case):
    from moni_align_amd import capi
    pats = case[3]
    halves = [pats[0::2], pats[1::2]]
    ctxs = [capi.Ctx(rig.idx), capi.Ctx(rig.idx)]
    try:
        def work(k):
            return [ctxs[k].loci_batch(*lm.ragged(halves[k]), strands=2, lift=1 - k, max_walk=0 if k else 8) for _ in range(4)]
        with ThreadPoolExecutor(2) as ex:
            outs = list(ex.map(work, (0, 1)))
        for k in (0, 1):
            lo.check_against_brute(rig.text, halves[k], outs[k][0], 2, 0 if k else 8, rig.fi.seq_starts, None if k else rig.keymap)
            for o in outs[k][1:]:
                assert all(np.array_equal(a, b) for a, b in zip(o, outs[k][0]))
    finally:
        for c in ctxs:
            c.close()


def test_agrees_with_locate_and_seqcount_on_the_same_context(rig, case):
    """the routes a caller had before: every occurrence listed by moni_locate and sorted on the host; the per-sequence table of moni_seqcount"""
    pats = case[3]
    n_seq = len(rig.fi.seq_starts) - 1
    lres, pos, sq, so = rig.ctx.locate_batch(*lm.ragged(pats), strands=2, max_occ=1 << 20)
    sres, counts = rig.ctx.seqcount_batch(*lm.ragged(pats), strands=2)
    res, lpos, lseq, lseq_off, support = rig.ctx.loci_batch(*lm.ragged(pats), strands=2, lift=0)
    for k in ("count", "sa_lo", "matched"):
        assert np.array_equal(lres[k], res[k]) and np.array_equal(sres[k], res[k]), k
    assert np.array_equal(sres["walked"], res["walked"]) and np.array_equal(sres["n_segs"], res["n_segs"])
    for t, r in enumerate(res):
        a, k = int(r["loci_off"]), int(r["n_loci"])
        la, lk = int(lres[t]["occ_off"]), int(lres[t]["n_occ"])
        assert k == lk == int(r["count"])
        order = np.argsort(pos[la:la + lk], kind="stable")
        assert np.array_equal(lpos[a:a + k], pos[la:la + lk][order]) and np.array_equal(lseq[a:a + k], sq[la:la + lk][order]) and np.array_equal(lseq_off[a:a + k], so[la:la + lk][order])
        assert np.array_equal(np.bincount(lseq[a:a + k], minlength=n_seq).astype(np.uint64), counts[t]), t
