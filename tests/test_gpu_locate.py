"""Exact-match count and locate on the GPU: count_kernel, the scan and locate_walk_kernel through the C ABI (Ctx.locate_batch / locate_run +
locate_fetch) against brute force that shares no code with the library - the count by direct search of the text, the positions and their order
from a naive suffix array, the coordinates from numpy.searchsorted on the sequence starts; every listed position is also checked to hold the
pattern.  A parity check: no tolerance."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import locate_model as lm

pytestmark = pytest.mark.gpu


class Rig:
    def __init__(self, fi, without_lcp=False):
        from moni_align_amd import capi
        self.fi = fi
        self.text = fi.text.tobytes()
        self.idx = capi.Index(fi=fi, device=0, without_lcp=without_lcp)
        self.ctx = capi.Ctx(self.idx)

    def check(self, pats, strands, max_occ, rank_of=None, limit=None, ctx=None):
        out = (ctx or self.ctx).locate_batch(*lm.ragged(pats), strands=strands, max_occ=max_occ)
        lm.check_against_brute(self.text, pats, *out, strands, max_occ, self.fi.seq_starts, rank_of, limit)
        return out

    def close(self):
        self.ctx.close()
        self.idx.close()


@pytest.fixture(scope="module")
def case():
    return lm.planted_case()


@pytest.fixture(scope="module")
def rig(case):
    r = Rig(case[0])
    yield r
    r.close()


@pytest.fixture(scope="module")
def rank_of(case):
    sa = lm.naive_sa(case[1])
    inv = [0] * len(sa)
    for k, x in enumerate(sa):
        inv[x] = k
    return inv


@pytest.mark.parametrize("strands,max_occ", [(1, 0), (1, 3), (2, 1000), (2, 1)])
def test_patterns_against_brute_force(rig, case, rank_of, strands, max_occ):
    """lengths 1, 2, 7, 8, 9, 31, 32, 33, 150 and a whole sequence; patterns that die at the first, a middle and the last step; absent bytes, bytes
    <= 1, lower case, N against N (a letter without a hot slot: the general path); the caps"""
    pats = case[2]
    res, pos, sq, so = rig.check(pats, strands, max_occ, rank_of)
    c = rig.ctx.counters()
    assert int(c[0]) > 0 and int(c[3]) > 0 and int(c[1]) <= 2 * int(c[0]) + int(c[0])
    assert int(c[2]) == int((res["n_occ"].astype(np.int64) - 1).clip(min=0).sum())          # n_occ - 1 phi steps per task
    unit = res[19 * strands]
    assert int(unit["count"]) >= 9 and int(unit["matched"]) == 40
    if max_occ == 0:                                             # count only: no position, no walk
        assert len(pos) == 0 and not res["n_occ"].any() and int(c[2]) == 0
    if max_occ == 3:                                             # the cap bites: the count stays exact, the list is the three highest ranks
        assert int(unit["n_occ"]) == 3
    for k, want in ((24, 0), (25, 0), (26, 0), (27, 19), (28, 39), (29, 39), (30, 19)):          # empty; an absent byte last, middle, first; dead at the last and a middle step
        assert int(res["count"][k * strands]) == 0 and int(res["matched"][k * strands]) == want, k
    assert rig.ctx.kernel_ms(0) > 0 and rig.ctx.kernel_ms(6) > 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_batch_sizes(rig, case, n):
    """block and wave tails, ragged lengths inside one 64-task block (the patterns in turn, from another start for every size)"""
    pats = case[2]
    batch = [pats[(7 * n + k) % len(pats)] for k in range(n)]
    rig.check(batch, 2, 4)
    rig.check(batch, 1, 2)


def test_empty_batch(rig):
    res, pos, sq, so = rig.ctx.locate_batch(np.zeros(0, np.uint8), np.zeros(1, np.uint64), strands=2, max_occ=5)
    assert len(res) == 0 and len(pos) == 0 and len(sq) == 0 and len(so) == 0
    res, pos, sq, so = rig.check([b"", b""], 2, 5)               # empty patterns: no occurrence
    assert not res["count"].any() and not res["matched"].any() and len(pos) == 0


def test_strand_1_is_the_forward_search_of_the_reverse_complement(rig, case):
    pats = case[2]
    both = rig.ctx.locate_batch(*lm.ragged(pats), strands=2, max_occ=6)
    fwd = rig.ctx.locate_batch(*lm.ragged([lm.revcomp(p) for p in pats]), strands=1, max_occ=6)
    for k in ("count", "sa_lo", "n_occ", "matched"):
        assert np.array_equal(both[0][k][1::2], fwd[0][k]), k
    for t in range(len(pats)):
        a, b = both[0][2 * t + 1], fwd[0][t]
        assert np.array_equal(both[1][int(a["occ_off"]):int(a["occ_off"]) + int(a["n_occ"])], fwd[1][int(b["occ_off"]):int(b["occ_off"]) + int(b["n_occ"])])
    assert int(both[0]["count"][-1]) >= 9 and int(both[0]["count"][-2]) == 0          # the last pattern is the planted unit's reverse complement


def test_index_without_lcp_samples(case, rank_of):
    r = Rig(case[0], without_lcp=True)
    try:
        r.check(case[2], 2, 7, rank_of)
    finally:
        r.close()


def test_long_runs_and_cold_letters():
    """a run of 4095 or more (the general path over rows / cr / recs), intervals that span it, N - a letter without a hot slot - at either end"""
    from tests.test_host_sim import long_run_case
    fi, reads = long_run_case()
    reads = [x.tobytes() for x in reads]
    r = Rig(fi)
    try:
        text = r.text
        at = text.find(b"NNNN")
        assert at > 40
        pats = [x[100:130] for x in reads[:60]] + reads[:10] + [text[a:a + 60] for a in range(0, 60000, 3000)]
        pats += [b"C" + text[13:53], text[12:53], text[13:33], b"N", b"NNNN", b"ANNNN", b"NNNNN", text[at - 20:at + 24], text[at - 1:at + 1], text[at + 3:at + 12]]
        res, pos, sq, so = r.check(pats, 2, 8, limit=4000)
        c = r.ctx.counters()
        assert int(c[3]) > 0 and int(res["count"].max()) >= 4095
        res, _, _, _ = r.check(pats + [b"C", b"CA"], 1, 0)          # (counts alone: a letter with 129 k occurrences is not ranked by brute force)
        assert int(res["count"][len(pats) - 7]) == 48 and int(res["count"][len(pats)]) >= 100000          # "N": 12 groups of four
    finally:
        r.close()


def test_run_fetch_after_swaps(rig, case):
    """locate_fetch takes its sizes from the run, whichever calls made the batch resident: batches of different sizes parked and recalled"""
    from moni_align_amd import capi
    pats = case[2]
    big, small = pats[:40], pats[40:] + [b""]
    cx = capi.Ctx(rig.idx)
    try:
        assert cx._L.moni_locate_fetch(cx._h, None, None, None, None) == -22 and cx._L.moni_locate_sizes(cx._h, None, None) == -22          # nothing was run yet
        p = cx._locate_params(1, 0)
        assert cx._L.moni_locate_run(cx._h, ctypes.byref(p)) == -22                                                                         # no batch is resident
        cx.upload(*lm.ragged(big))
        cx.swap(0)                                   # big parked
        cx.upload(*lm.ragged(small))
        cx.swap(0)                                   # big resident again, small parked
        cx.locate_run(strands=2, max_occ=5)
        out = cx.locate_fetch()
        lm.check_against_brute(rig.text, big, *out, 2, 5, rig.fi.seq_starts)
        only = cx.locate_fetch(want_occ=False)
        assert np.array_equal(only[0], out[0]) and len(only[1]) == 0
        cx.swap(0)                                   # small resident: the last run's results are gone with its batch
        with pytest.raises(RuntimeError):
            cx.locate_fetch()
        cx.locate_run(strands=1, max_occ=0)
        out = cx.locate_fetch()
        lm.check_against_brute(rig.text, small, *out, 1, 0, rig.fi.seq_starts)
        cx.locate_run(strands=1, max_occ=100000)     # the occurrence buffer grows
        out = cx.locate_fetch()
        lm.check_against_brute(rig.text, small, *out, 1, 100000, rig.fi.seq_starts)
        before = cx.ms_query_batch(*lm.ragged(big))  # uploads inside the call; the other walks' workspaces are shared
        cx.locate_run(strands=2, max_occ=2)
        lm.check_against_brute(rig.text, big, *cx.locate_fetch(), 2, 2, rig.fi.seq_starts)
        assert np.array_equal(cx.ms_query_batch(*lm.ragged(big)), before)
    finally:
        cx.close()


def test_two_contexts_with_batches_in_flight(rig, case):
    from moni_align_amd import capi
    pats = case[2]
    halves = [pats[0::2], pats[1::2]]
    ctxs = [capi.Ctx(rig.idx), capi.Ctx(rig.idx)]
    try:
        def work(k):
            return [ctxs[k].locate_batch(*lm.ragged(halves[k]), strands=2, max_occ=3 + k) for _ in range(4)]
        with ThreadPoolExecutor(2) as ex:
            outs = list(ex.map(work, (0, 1)))
        for k in (0, 1):
            lm.check_against_brute(rig.text, halves[k], *outs[k][0], 2, 3 + k, rig.fi.seq_starts)
            for o in outs[k][1:]:
                assert all(np.array_equal(a, b) for a, b in zip(o, outs[k][0]))
        ctxs[0].upload(*lm.ragged(halves[0]))        # run on one, run on the other, fetch in the other order
        ctxs[1].upload(*lm.ragged(halves[1]))
        ctxs[0].locate_run(2, 3)
        ctxs[1].locate_run(2, 4)
        b = ctxs[1].locate_fetch()
        a = ctxs[0].locate_fetch()
        assert all(np.array_equal(x, y) for x, y in zip(a, outs[0][0])) and all(np.array_equal(x, y) for x, y in zip(b, outs[1][0]))
    finally:
        for c in ctxs:
            c.close()


def test_invalid_parameters(rig, case):
    from moni_align_amd import capi
    L = rig.ctx._L
    b, keep = rig.ctx._batch(*lm.ragged(case[2][:3]))
    res = np.zeros(6, dtype=capi.LOCATE_RES_DTYPE)
    rig.ctx.upload(*lm.ragged(case[2][:3]))
    for strands, r0, r1 in ((0, 0, 0), (3, 0, 0), (1, 1, 0), (2, 0, 7)):
        p = capi.LocateParamsC(strands, 4, (r0, r1))
        assert L.moni_locate_run(rig.ctx._h, ctypes.byref(p)) == -22
        assert L.moni_locate_batch(rig.ctx._h, ctypes.byref(b), ctypes.byref(p), res.ctypes.data, None, None, None, None) == -22
    assert L.moni_locate_run(rig.ctx._h, None) == -22
    p = capi.LocateParamsC(2, 4, (0, 0))
    n = ctypes.c_uint64()
    assert L.moni_locate_batch(rig.ctx._h, ctypes.byref(b), ctypes.byref(p), res.ctypes.data, None, None, None, ctypes.byref(n)) == 0          # pos, seq and seq_off may be NULL
    assert n.value == int(res["n_occ"].sum()) > 0
