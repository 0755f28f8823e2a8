"""Pseudo-matching lengths on the GPU: the lengths, read_max and read_hits of Ctx.pml_batch / pml_run + pml_fetch and the text of
`moni-hip-align --pseudo-ms` equal the plain-Python model (tests/pml_model.py).  A parity check: no tolerance."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import pml_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "moni_align_amd", "host", "moni-hip-align")


class Rig:
    def __init__(self, fi):
        from moni_align_amd import capi
        self.model = pml_model.PmlModel(fi)
        self.idx = capi.Index(fi=fi, device=0)
        self.ctx = capi.Ctx(self.idx)

    def check(self, reads, thr=25, want=None):
        """pml_batch against the model; returns the model's per-read lengths"""
        ls = want if want is not None else [self.model.query(r) for r in reads]
        seq, offs = pml_model.ragged(reads)
        ln, mx, hits = self.ctx.pml_batch(seq, offs, thr)
        flat = np.array([x for l in ls for x in l], dtype=np.uint32)
        if not np.array_equal(ln, flat):          # the first differing read, for the log
            for i, l in enumerate(ls):
                g = ln[int(offs[i]):int(offs[i + 1])].tolist()
                assert g == l, "read %d (length %d): got %r want %r" % (i, len(l), g, l)
        assert mx.tolist() == [max(l) if l else 0 for l in ls]
        assert hits.tolist() == [sum(1 for x in l if x >= thr) for l in ls]
        return ls

    def close(self):
        self.ctx.close()
        self.idx.close()


@pytest.fixture(scope="module")
def rig(medium_case):
    r = Rig(medium_case.fi)
    yield r
    r.close()


@pytest.fixture(scope="module")
def sim2000(medium_case):
    return [r.tobytes() for r in medium_case.synth.make_reads(medium_case.pg, 2000, 150, seed=61, sub_rate=0.02, indel_rate=0.003)]


@pytest.fixture(scope="module")
def sim2000_want(rig, sim2000):
    return [rig.model.query(r) for r in sim2000]


def test_simulated_reads(rig, sim2000, sim2000_want):
    flat = np.array([x for l in sim2000_want for x in l])
    assert int((flat >= 25).sum()) * 10 >= len(flat)          # the comparison is not vacuous
    rig.check(sim2000, 25, sim2000_want)
    seq, offs = pml_model.ragged(sim2000)
    _, _, hits = rig.ctx.pml_batch(seq, offs, 1)
    assert hits.tolist() == [sum(1 for x in l if x >= 1) for l in sim2000_want]
    _, _, hits = rig.ctx.pml_batch(seq, offs, 10000)
    assert not hits.any()                                      # no read is that long
    _, _, hits = rig.ctx.pml_batch(seq, offs, 0)
    assert hits.tolist() == [150] * 2000                       # every offset has a length >= 0
    c = rig.ctx.counters()
    assert int(c[0]) == 2000 * 150 and 0 < int(c[1]) < int(c[0])
    assert rig.ctx.kernel_ms(6) > 0 and rig.ctx.kernel_ms(0) > 0


def test_ragged_batch(rig, medium_case):
    text = medium_case.text
    base = [r.tobytes() for r in medium_case.synth.make_reads(medium_case.pg, 3, 2048, seed=62, sub_rate=0.02, indel_rate=0.0005)]
    reads = []
    for k, L in enumerate((0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 2048)):          # pattern-word and block edges
        reads.append(base[k % 3][:L])
    reads.append(b"N" * 60)
    reads.append(text[2000:2150].lower())
    reads.append(text[3000:3070] + b"N" + text[3071:3150])
    reads.append(text[100:400])                                                                  # an exact 300-mer
    reads.append(pml_model.mixed_case(text[5000:5150]))                                          # absent letters above the alphabet, then present ones
    reads += [r.tobytes() for r in medium_case.synth.make_reads(medium_case.pg, 21, 150, seed=63, sub_rate=0.02, indel_rate=0.003)]
    assert len(reads) == 40
    ls = rig.check(reads)
    assert ls[14] == [0] * 60 and ls[15] == [0] * 150 and ls[16][70] == 0
    assert ls[17][0] >= 25 and ls[13] and max(ls[13]) >= 25
    assert ls[18][40] == 0 and ls[18][41] == 0 and ls[18][39] == 0 and max(ls[18]) >= 25
    rig.check(reads[::-1])                                                                       # the long read in another block, the empty one last


def test_long_runs_and_cold_letters():
    from tests.test_host_sim import long_run_case
    fi, reads = long_run_case()
    r = Rig(fi)
    try:
        ls = r.check([x.tobytes() for x in reads])
        assert max(max(l) for l in ls) >= 25
    finally:
        r.close()


def test_batch_sizes(rig, sim2000, sim2000_want):
    ln, mx, hits = rig.ctx.pml_batch(np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    assert len(ln) == 0 and len(mx) == 0 and len(hits) == 0
    for n in (1, 64, 65, 257):                                 # block and wave tails
        rig.check(sim2000[100:100 + n], 25, sim2000_want[100:100 + n])


def test_run_fetch_and_workspaces(rig, sim2000, sim2000_want):
    from moni_align_amd import capi
    reads, want = sim2000[:500], sim2000_want[:500]
    seq, offs = pml_model.ragged(reads)
    fresh = capi.Ctx(rig.idx)
    try:
        assert fresh._L.moni_pml_fetch(fresh._h, None, None, None) != 0          # nothing was run on this context yet
        before = fresh.ms_query_batch(seq, offs)
        ln, mx, hits = fresh.pml_batch(seq, offs, 25)
        fresh.upload(seq, offs)
        with pytest.raises(RuntimeError):
            fresh.pml_fetch()                                                    # another batch was made resident since the last run
        fresh.pml_run(25)
        ln2, mx2, hits2 = fresh.pml_fetch()
        assert np.array_equal(ln2, ln) and np.array_equal(mx2, mx) and np.array_equal(hits2, hits)
        assert ln.tolist() == [x for l in want for x in l]
        none, mx3, _ = fresh.pml_fetch(want_lengths=False)
        assert none is None and np.array_equal(mx3, mx)
        fresh.pml_run(40)                                                        # another thr changes read_hits alone
        ln4, mx4, hits4 = fresh.pml_fetch()
        assert np.array_equal(ln4, ln) and np.array_equal(mx4, mx)
        assert hits4.tolist() == [sum(1 for x in l if x >= 40) for l in want] and not np.array_equal(hits4, hits)
        assert np.array_equal(fresh.ms_query_batch(seq, offs), before)           # the pointer walk's workspaces are as they were
        b, keep = fresh._batch(seq, offs)
        assert fresh._L.moni_pml_batch(fresh._h, ctypes.byref(b), 25, None, None, None) != 0   # all three outputs NULL
    finally:
        fresh.close()


def test_fetch_after_swap_and_after_other_uploads(rig, sim2000, sim2000_want):
    """pml_fetch takes its sizes from the run, whichever calls made the batch resident: batches of different sizes parked and recalled with
    swap(), and a batch that another *_batch call uploaded"""
    from moni_align_amd import capi
    big, big_want = sim2000[:300], sim2000_want[:300]
    small, small_want = sim2000[300:307] + [b""], sim2000_want[300:307] + [[]]
    flat = lambda ls: [x for l in ls for x in l]
    cx = capi.Ctx(rig.idx)
    try:
        cx.upload(*pml_model.ragged(big))
        cx.swap(0)                                   # big parked
        cx.upload(*pml_model.ragged(small))
        cx.swap(0)                                   # big resident again, small parked
        cx.pml_run(25)
        ln, mx, hits = cx.pml_fetch()
        assert ln.tolist() == flat(big_want) and mx.tolist() == [max(l) for l in big_want] and len(hits) == 300
        cx.swap(0)                                   # small resident: the last run's results are gone with its batch
        with pytest.raises(RuntimeError):
            cx.pml_fetch()
        cx.pml_run(25)
        ln, mx, hits = cx.pml_fetch()
        assert ln.tolist() == flat(small_want) and mx.tolist() == [max(l) if l else 0 for l in small_want] and len(hits) == 8
    finally:
        cx.close()
    cx = capi.Ctx(rig.idx)
    try:
        cx.ms_query_batch(*pml_model.ragged(big))    # uploads inside the call
        cx.pml_run(25)
        ln, mx, hits = cx.pml_fetch()
        assert ln.tolist() == flat(big_want) and len(mx) == 300
    finally:
        cx.close()


def test_cli_pseudo_ms(medium_case, tmp_path):
    import __graft_entry__
    __graft_entry__.build()
    N = 2500
    reads = medium_case.synth.make_reads(medium_case.pg, N, 150, seed=64, sub_rate=0.02, indel_rate=0.003)
    fq = str(tmp_path / "reads.fastq")
    medium_case.synth.write_fastq(fq, reads)
    out = str(tmp_path / "pml")
    r = subprocess.run([EXE, medium_case.path[:-4], "-p", fq, "-o", out, "--pseudo-ms", "--gpu-batch", "900", "-t", "4"], capture_output=True)
    assert r.returncode == 0, r.stderr
    model = pml_model.PmlModel(medium_case.fi)
    want = pml_model.render([model.query(x.tobytes()) for x in reads])
    got = open(out + ".pseudo_lengths", "rb").read()
    assert got == want
    assert b">899\n" in got and b">900\n" in got and b">2499\n" in got          # the numbering crosses the batches' borders
