"""Read screening on the GPU: the records of Ctx.screen_batch / screen_run + screen_fetch equal the plain-Python definition
(tests/screen_model.py) field for field.  A parity check: no tolerance."""
import ctypes

import numpy as np
import pytest

from tests import pml_model, screen_model as sm
from tests.test_screen_model import chimeras

pytestmark = pytest.mark.gpu

P = sm.Params
EINVAL = -22


class Rig:
    def __init__(self, fi):
        from moni_align_amd import capi
        self.capi = capi
        self.model = pml_model.PmlModel(fi)
        self.idx = capi.Index(fi=fi, device=0)
        self.ctx = capi.Ctx(self.idx)
        self._walked = {}

    def walked(self, reads):
        """both strands' lengths of every read, walked once per distinct read"""
        for r in reads:
            if r not in self._walked:
                self._walked[r] = sm.walk_read(self.model, r)
        return [self._walked[r] for r in reads]

    def want(self, reads, p):
        return [sm.screen_read(self.model, r, p, walked=w) for r, w in zip(reads, self.walked(reads))]

    def check(self, reads, p=P(), ctx=None):
        """screen_batch against the model; returns the model's records"""
        want = self.want(reads, p)
        seq, offs = pml_model.ragged(reads)
        res = (ctx or self.ctx).screen_batch(seq, offs, **p._asdict())
        got = sm.as_tuples(res)
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, "read %d (length %d) %r: got %r want %r" % (i, len(reads[i]), p, g, w)
        return want

    def close(self):
        self.ctx.close()
        self.idx.close()


@pytest.fixture(scope="module")
def rig(medium_case):
    r = Rig(medium_case.fi)
    yield r
    r.close()


@pytest.fixture(scope="module")
def sim257(medium_case):
    return [r.tobytes() for r in medium_case.synth.make_reads(medium_case.pg, 257, 150, seed=81, sub_rate=0.02, indel_rate=0.003)]


@pytest.fixture(scope="module")
def ragged_reads(medium_case):
    """pattern-word, window and min_win edges; N runs, lower case, mixed case, an exact 300-mer, the chimeras"""
    text = medium_case.text
    base = [r.tobytes() for r in medium_case.synth.make_reads(medium_case.pg, 3, 2048, seed=82, sub_rate=0.02, indel_rate=0.0005)]
    reads = [base[k % 3][:L] for k, L in enumerate((0, 1, 7, 8, 9, 24, 25, 49, 50, 51, 74, 75, 100, 255, 256, 257, 2048))]
    reads.append(b"N" * 60)
    reads.append(text[2000:2150].lower())
    reads.append(text[3000:3070] + b"NNN" + text[3073:3150])
    reads.append(text[100:400])
    reads.append(pml_model.mixed_case(text[5000:5150]))
    reads += chimeras(medium_case)
    return reads


def test_simulated_reads_counters_and_time(rig, sim257):
    want = rig.check(sim257)
    assert sm.n_present(want) * 100 >= 95 * len(want)                      # the comparison is not vacuous
    assert any(r[4] & sm.STRAND1 for r in want) and any(not r[4] & sm.STRAND1 for r in want)
    c = rig.ctx.counters()
    assert int(c[0]) == 4 * 257 * 150                                       # 2 * strands steps per base
    assert int(c[2]) == sum(rig.model.walk(r)[1] for r in sim257)           # the P0 lanes jump where the model's walk does
    assert 0 < int(c[2]) < int(c[1]) < int(c[0])
    assert rig.ctx.kernel_ms(0) > 0 and rig.ctx.kernel_ms(6) > 0
    rig.check(sim257, P(strands=1))
    assert int(rig.ctx.counters()[0]) == 2 * 257 * 150


def test_random_reads_are_absent(rig):
    rng = np.random.default_rng(83)
    rnd = [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=150)].tobytes() for _ in range(100)]
    assert sm.n_present(rig.check(rnd)) * 100 <= 5 * len(rnd)


def test_ragged_batch(rig, ragged_reads):
    want = rig.check(ragged_reads)
    assert want[0] == (0, (0, 0), (0, 0), (0, 0), sm.SHORT) and all(w[4] & sm.SHORT for w in want[:6]) and not want[6][4] & sm.SHORT      # lengths 0 .. 24, then 25
    assert want[16][0] == 41 and want[16][4] & sm.PRESENT                                                                              # 2048 = 40 windows + 48 offsets
    assert want[17][4] == 0 and want[17][3] == (0, 0)                                                                                  # N runs: nothing matches
    exact = want[20]
    assert exact[3][0] > sm.BINS and exact[2][0] == 50 and exact[4] == sm.PRESENT          # lengths far above the clip: max_pml is not clipped, D is the window length
    rig.check(ragged_reads[::-1])                                                          # the long read in another block, the empty one last
    rig.check(ragged_reads, P(strands=1))


def test_chimeras(rig, medium_case):
    reads = chimeras(medium_case)
    for batch in (reads, reads[::-1]):
        want = rig.check(batch, P(64, 32))
        by_read = dict(zip(batch, want))
        assert not by_read[reads[0]][4] & sm.PRESENT and by_read[reads[1]][4] == sm.PRESENT and by_read[reads[2]][4] == sm.PRESENT | sm.STRAND1


def test_long_runs_and_cold_letters():
    from tests.test_host_sim import long_run_case
    fi, reads = long_run_case()
    r = Rig(fi)
    try:
        want = r.check([x.tobytes() for x in reads[:130]])
        assert sm.n_present(want) >= 65
    finally:
        r.close()


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 63, 64, 65, 257])
def test_batch_sizes(rig, sim257, n):
    """the quad, wave and block tails of a launch with four lanes per read (two with one strand)"""
    rig.check(sim257[:n])
    rig.check(sim257[:n], P(strands=1))


@pytest.mark.parametrize("p", [P(8, 1), P(8, 8), P(50, 1), P(50, 50), P(64, 32), P(64, 64), P(65535, 1), P(65535, 65535),
                               P(ks_num=1, ks_den=2), P(ks_num=1, ks_den=1), P(64, 32, 1, 2), P(8, 1, 65535, 65535), P(150, 75, 3, 4, 1)])
def test_window_shapes_and_thresholds(rig, ragged_reads, sim257, p):
    want = rig.check(ragged_reads + sim257[:40], p)
    if p.window == 65535:
        assert all(w[0] == (1 if len(r) >= p.min_win else 0) for r, w in zip(ragged_reads, want))          # one window per read


def test_parameter_errors(rig, sim257):
    seq, offs = pml_model.ragged(sim257[:4])
    capi = rig.capi
    b, keep = rig.ctx._batch(seq, offs)
    res = np.zeros(4, dtype=capi.SCREEN_RES_DTYPE)
    bad = [dict(window=7), dict(window=65536), dict(min_win=0), dict(min_win=51), dict(window=8, min_win=9), dict(ks_num=0), dict(ks_num=5), dict(ks_den=0),
           dict(ks_num=1, ks_den=65536), dict(strands=0), dict(strands=3)]
    rig.ctx.upload(seq, offs)
    for kw in bad:
        p = rig.ctx._screen_params(kw)
        assert rig.ctx._L.moni_screen_batch(rig.ctx._h, ctypes.byref(b), ctypes.byref(p), res.ctypes.data) == EINVAL, kw
        assert rig.ctx._L.moni_screen_run(rig.ctx._h, ctypes.byref(p)) == EINVAL, kw
    p = rig.ctx._screen_params({})
    p.reserved[1] = 1
    assert rig.ctx._L.moni_screen_run(rig.ctx._h, ctypes.byref(p)) == EINVAL
    assert rig.ctx._L.moni_screen_run(rig.ctx._h, None) == EINVAL
    assert rig.ctx._L.moni_screen_batch(rig.ctx._h, ctypes.byref(b), ctypes.byref(rig.ctx._screen_params({})), None) == EINVAL          # reads, and nowhere to put their records
    d = rig.ctx._screen_params({})
    assert (d.window, d.min_win, d.ks_num, d.ks_den, d.strands) == (50, 25, 1, 4, 2)


def test_run_fetch_invalidation_and_workspaces(rig, sim257):
    capi = rig.capi
    reads = sim257[:200]
    want = rig.want(reads, P())
    seq, offs = pml_model.ragged(reads)
    cx = capi.Ctx(rig.idx)
    try:
        assert cx._L.moni_screen_fetch(cx._h, None) == EINVAL and cx._L.moni_screen_sizes(cx._h, None) == EINVAL          # nothing was run on this context yet
        assert cx._L.moni_screen_run(cx._h, ctypes.byref(cx._screen_params({}))) == EINVAL                                # no resident batch
        ms_before = cx.ms_query_batch(seq, offs)
        pml_before = cx.pml_batch(seq, offs, 25)
        cx.screen_run()
        assert sm.as_tuples(cx.screen_fetch()) == want
        assert sm.as_tuples(cx.screen_fetch()) == want                                                                     # fetching takes nothing away
        cx.screen_run(window=64, min_win=32)
        assert sm.as_tuples(cx.screen_fetch()) == rig.want(reads, P(64, 32))
        cx.pml_run(25)                                                                                                     # the PML workspaces are as they were
        for a, b in zip(cx.pml_fetch(), pml_before):
            assert np.array_equal(a, b)
        assert sm.as_tuples(cx.screen_fetch()) == rig.want(reads, P(64, 32))                                               # ... and a PML run leaves the records alone
        assert np.array_equal(cx.ms_query_batch(seq, offs), ms_before)                                                     # uploads: the records are gone
        with pytest.raises(RuntimeError):
            cx.screen_fetch()
        for a, b in zip(cx.pml_batch(seq, offs, 25), pml_before):
            assert np.array_equal(a, b)
        cx.screen_run()
        cx.upload(*pml_model.ragged(reads[:7]))
        with pytest.raises(RuntimeError):
            cx.screen_fetch()                                                                                              # another batch was made resident
        cx.screen_run()
        assert sm.as_tuples(cx.screen_fetch()) == want[:7]
        cx.swap(0)                                                                                                         # parked: nothing resident
        with pytest.raises(RuntimeError):
            cx.screen_fetch()
        cx.swap(0)
        with pytest.raises(RuntimeError):
            cx.screen_fetch()                                                                                              # resident again, but not the run's results
        cx.screen_run(strands=1)
        assert sm.as_tuples(cx.screen_fetch()) == rig.want(reads[:7], P(strands=1))
    finally:
        cx.close()
