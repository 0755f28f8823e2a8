"""k-mismatch count and locate on the GPU: approx_exact_kernel, approx_tree_kernel, the scans, the gather and approx_walk_kernel through the C ABI
(Ctx.approx_batch / approx_run + approx_fetch + approx_sizes) against brute force that shares no code with the library - numpy sliding-window
compares of the text, the A / C / G / T rule on the text bytes, positions binned with numpy.searchsorted.  A parity check: no tolerance.  Where a
task has more hits than max_hits the kept ones are checked to be true hits (which of them are kept is not specified); the step counter is the
plain-Python model's."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import approx_model as am
from tests import locate_model as lm

pytestmark = pytest.mark.gpu


class Rig:
    def __init__(self, fi, without_lcp=False):
        from moni_align_amd import capi
        self.fi = fi
        self.text = fi.text.tobytes()
        self.idx = capi.Index(fi=fi, device=0, without_lcp=without_lcp)
        self.ctx = capi.Ctx(self.idx)

    def verify(self, pats, out, strands, k, max_hits, max_occ, counters=None):
        res, hits, pos, sq, so = out
        am.check_against_brute(self.text, pats, res, hits, pos, sq, so, strands, k, max_hits, max_occ, self.fi.seq_starts)
        if counters is not None:
            assert int(counters[2]) == int((hits["n_occ"].astype(np.int64) - 1).clip(min=0).sum())

    def check(self, pats, strands, k, max_hits, max_occ, chunk_len=16, ctx=None):
        ctx = ctx or self.ctx
        out = ctx.approx_batch(*lm.ragged(pats), strands=strands, k=k, max_hits=max_hits, max_occ=max_occ, chunk_len=chunk_len)
        self.verify(pats, out, strands, k, max_hits, max_occ, ctx.counters())
        return out

    def close(self):
        self.ctx.close()
        self.idx.close()


@pytest.fixture(scope="module")
def case():
    return am.approx_patterns()


@pytest.fixture(scope="module")
def model(case):
    return am.ApproxModel(case[0])


@pytest.fixture(scope="module")
def rig(case):
    r = Rig(case[0])
    yield r
    r.close()


@pytest.mark.parametrize("strands,k,max_hits,max_occ", [(1, 0, 0, 0), (1, 1, 8, 4), (2, 2, 64, 1000), (2, 3, 4, 1)])
def test_patterns_against_brute_force(rig, case, model, strands, k, max_hits, max_occ):
    fi, text, pats, marks = case
    res, hits, pos, sq, so = rig.check(pats, strands, k, max_hits, max_occ)
    c = rig.ctx.counters()
    assert int(c[0]) == model.approx_batch(pats, strands, k, 0, 0)[5]          # every attempted (node, letter) step once
    assert int(c[1]) > 0 and int(c[3]) > 0 and res["complete"].all()
    assert not res["cnt"][:, k + 1:].any()
    assert rig.ctx.kernel_ms(0) > 0 and rig.ctx.kernel_ms(6) >= rig.ctx.kernel_ms(0) and (k == 0 or rig.ctx.kernel_ms(3) > 0)
    t = lambda name: marks[name] * strands
    assert [int(res["matched"][t(n)]) for n in ("dies first", "dies middle", "dies last")] == [0, 19, 39]
    if k:
        for name in ("absent byte", "byte <= 1", "lower case", "dies first", "dies middle", "dies last", "N in pattern"):
            assert int(res["cnt"][t(name), 0]) == 0 and int(res["cnt"][t(name), 1]) >= 1, name
    if k == 3:
        assert (res["cnt"] > 0).all(axis=1).any() and (res["n_hits"] > max_hits).any() and int(res["n_kept"].max()) == max_hits


@pytest.mark.parametrize("chunk_len", [1, 16, 1 << 20])
def test_pieces(rig, case, model, chunk_len):
    fi, text, pats, marks = case
    rig.check(pats, 2, 2, 64, 1000, chunk_len)
    assert int(rig.ctx.counters()[0]) == model.approx_batch(pats, 2, 2, 0, 0)[5]          # the same tree whoever walks it


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_batch_sizes(rig, case, n):
    """block and wave tails of the task and the piece kernels (the patterns in turn, from another start for every size)"""
    pats = case[2]
    batch = [pats[(7 * n + j) % len(pats)] for j in range(n)]
    rig.check(batch, 2, 1, 8, 2)
    rig.check(batch, 1, 2, 64, 0)


def test_k0_is_locate_and_leaves_it_fetchable(rig, case, model):
    pats = case[2]
    cx = rig.ctx
    lres, lpos, lsq, lso = cx.locate_batch(*lm.ragged(pats), strands=2, max_occ=5)
    cx.approx_run(strands=2, k=0, max_hits=1, max_occ=5)          # (over the batch locate_batch made resident)
    res, hits, pos, sq, so = cx.approx_fetch()
    assert np.array_equal(res["cnt"][:, 0], lres["count"]) and np.array_equal(res["matched"], lres["matched"]) and not res["cnt"][:, 1:].any()
    occ = lres["count"] > 0
    assert np.array_equal(res["n_hits"], occ.astype(np.uint64)) and np.array_equal(hits["sa_lo"], lres["sa_lo"][occ]) and np.array_equal(hits["count"], lres["count"][occ])
    assert np.array_equal(pos, lpos) and np.array_equal(sq, lsq) and np.array_equal(so, lso)
    again = cx.locate_fetch()                                     # the locate result of the context is still there
    assert np.array_equal(again[0], lres) and np.array_equal(again[1], lpos)
    assert int(cx.counters()[0]) == model.approx_batch(pats, 2, 0, 0, 0)[5]


def test_run_fetch_sizes_after_swap(rig, case):
    from moni_align_amd import capi
    pats = case[2]
    big, small = pats[:40], pats[40:] + [b""]
    cx = capi.Ctx(rig.idx)
    try:
        p = cx._approx_params(1, 1, 4, 2, 16, None)
        assert cx._L.moni_approx_fetch(cx._h, None, None, None, None, None) == -22 and cx._L.moni_approx_sizes(cx._h, None, None, None) == -22      # nothing was run yet
        assert cx._L.moni_approx_run(cx._h, ctypes.byref(p)) == -22                                                                              # no batch is resident
        cx.upload(*lm.ragged(big))
        cx.swap(0)                                   # big parked
        cx.upload(*lm.ragged(small))
        cx.swap(0)                                   # big resident again, small parked
        cx.approx_run(strands=2, k=2, max_hits=64, max_occ=3)
        out = cx.approx_fetch()
        assert cx.approx_sizes() == (2 * len(big), len(out[1]), len(out[2]))
        rig.verify(big, out, 2, 2, 64, 3, cx.counters())
        only = cx.approx_fetch(want_hits=False)
        assert np.array_equal(only[0], out[0]) and len(only[1]) == 0 and len(only[2]) == 0
        cx.swap(0)                                   # small resident: the last run's results are gone with its batch
        with pytest.raises(RuntimeError):
            cx.approx_fetch()
        cx.approx_run(strands=1, k=1, max_hits=8, max_occ=0)
        rig.verify(small, cx.approx_fetch(), 1, 1, 8, 0)
        cx.upload(*lm.ragged(big))                   # fetch after moni_reads_upload
        assert cx._L.moni_approx_fetch(cx._h, None, None, None, None, None) == -22 and cx._L.moni_approx_sizes(cx._h, None, None, None) == -22
    finally:
        cx.close()


def test_invalid_parameters(rig, case):
    from moni_align_amd import capi
    L = rig.ctx._L
    pats = case[2][:3]
    b, keep = rig.ctx._batch(*lm.ragged(pats))
    res = np.zeros(6, dtype=capi.APPROX_RES_DTYPE)
    rig.ctx.upload(*lm.ragged(pats))
    #                strands k max_hits max_occ chunk_len reserved
    for bad in ((0, 1, 0, 0, 16, 0), (3, 1, 0, 0, 16, 0), (1, 4, 0, 0, 16, 0), (1, 1, 0, 0, 0, 0), (1, 1, 0, 2, 16, 0), (2, 1, 4, 0, 16, 9)):
        p = capi.ApproxParamsC(*bad, 0)
        assert L.moni_approx_run(rig.ctx._h, ctypes.byref(p)) == -22, bad
        assert L.moni_approx_batch(rig.ctx._h, ctypes.byref(b), ctypes.byref(p), res.ctypes.data, None, None, None, None, None, None) == -22, bad
    assert L.moni_approx_run(rig.ctx._h, None) == -22
    p = capi.ApproxParamsC(2, 1, 4, 2, 16, 0, 0)
    assert L.moni_approx_batch(rig.ctx._h, ctypes.byref(b), ctypes.byref(p), res.ctypes.data, None, None, None, None, None, None) == 0          # the lists may be NULL
    assert int(res["cnt"].sum()) > 0
    d = capi.ApproxParamsC()
    L.moni_approx_params_default(ctypes.byref(d))
    assert (d.strands, d.k, d.max_hits, d.max_occ, d.chunk_len, d.reserved, d.max_steps) == (1, 1, 0, 0, capi.APPROX_CHUNK_LEN_DEFAULT, 0, capi.APPROX_MAX_STEPS_DEFAULT)


def test_empty_batch_and_empty_patterns(rig):
    res, hits, pos, sq, so = rig.ctx.approx_batch(np.zeros(0, np.uint8), np.zeros(1, np.uint64), strands=2, k=2, max_hits=4, max_occ=2)
    assert len(res) == 0 and len(hits) == 0 and len(pos) == 0
    res, hits, pos, sq, so = rig.check([b"", b""], 2, 3, 4, 2)
    assert not res["cnt"].any() and not res["n_hits"].any() and res["complete"].all() and len(hits) == 0


def test_max_steps_stops_a_piece(rig, case, model):
    fi, text, pats, marks = case
    full = rig.ctx.approx_batch(*lm.ragged(pats), strands=1, k=2, max_hits=0, max_occ=0, chunk_len=16, max_steps=0)[0]
    cut = rig.ctx.approx_batch(*lm.ragged(pats), strands=1, k=2, max_hits=0, max_occ=0, chunk_len=16, max_steps=40)[0]
    want = model.approx_batch(pats, 1, 2, 0, 0, 16, 40)
    for f in ("cnt", "n_hits", "complete", "matched"):           # the pieces are a function of the pattern and chunk_len: the model says where each stops
        assert np.array_equal(cut[f], want[0][f]), f
    assert int(rig.ctx.counters()[0]) == want[5]
    stopped = cut["complete"] == 0
    assert stopped.any() and not stopped.all() and (cut["cnt"] <= full["cnt"]).all() and (cut["n_hits"][stopped] < full["n_hits"][stopped]).any()
    assert np.array_equal(cut["cnt"][~stopped], full["cnt"][~stopped]) and full["complete"].all()


def test_index_without_lcp_samples(case):
    r = Rig(case[0], without_lcp=True)
    try:
        r.check(case[2], 2, 2, 64, 3)
    finally:
        r.close()


def test_two_contexts_from_two_threads(rig, case):
    from moni_align_amd import capi
    pats = case[2]
    halves = [pats[0::2], pats[1::2]]
    prm = [dict(strands=2, k=2, max_hits=64, max_occ=2), dict(strands=2, k=1, max_hits=8, max_occ=0)]
    ctxs = [capi.Ctx(rig.idx), capi.Ctx(rig.idx)]
    try:
        def work(j):
            return [ctxs[j].approx_batch(*lm.ragged(halves[j]), **prm[j]) for _ in range(4)]
        with ThreadPoolExecutor(2) as ex:
            outs = list(ex.map(work, (0, 1)))
        for j in (0, 1):
            rig.verify(halves[j], outs[j][0], prm[j]["strands"], prm[j]["k"], prm[j]["max_hits"], prm[j]["max_occ"])
            for o in outs[j][1:]:                                 # (which hits a full task keeps may change from run to run; the counts may not)
                assert all(np.array_equal(o[0][f], outs[j][0][0][f]) for f in ("cnt", "n_hits", "n_kept", "complete", "matched"))
    finally:
        for c in ctxs:
            c.close()
