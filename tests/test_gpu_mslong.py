"""Matching statistics of long patterns on the GPU: moni_ms_long_batch over the patterns and settings of tests/test_host_mslong.py, held to
OracleIndex.ms_lengths by the same checks (tests/mslong_model.py): the lengths at every position, every pointer a position of a match of that
length, the step counts and the flagged segments as the matching statistics predict them, no tolerance; with nothing cut, pointers equal to
moni_ms_lengths_batch's.  And `moni-hip-align --ms / --mems --split` against the run without --split."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import mslong_model as mm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "moni_align_amd", "host", "moni-hip-align")


class Rig:
    def __init__(self, fi, path):
        from moni_align_amd import capi
        from oracle import orc
        self.idx = capi.Index(fi=fi, device=0)
        self.ctx = capi.Ctx(self.idx)
        self.orc = orc.OracleIndex(path)
        self.text = fi.text.tobytes()
        self.n = int(fi.n)

    def __call__(self, seq, offs, seg_len, overlap):
        return self.ctx.ms_long_batch(seq, offs, seg_len, overlap)

    def check(self, pats, seg_len, overlap, want=None):
        return mm.check(self, self.orc, self.text, self.n, pats, seg_len, overlap, want)

    def close(self):
        self.ctx.close()
        self.idx.close()


@pytest.fixture(scope="module")
def rig(medium_case):
    r = Rig(medium_case.fi, medium_case.path)
    yield r
    r.close()


@pytest.fixture(scope="module")
def random_want(rig):
    pats = mm.random_batch()
    return pats, [rig.orc.ms_lengths(p) for p in pats]


@pytest.mark.parametrize("seg_len,overlap", mm.SETTINGS)
def test_ragged_batch(rig, medium_case, seg_len, overlap):
    """(c) + (d): edge lengths, a 20 000-base pattern, N / lower case / an absent byte at segment edges and inside an overlap; ragged offsets"""
    pats = mm.ragged_batch(medium_case, seg_len, overlap)
    st, _, want = rig.check(pats, seg_len, overlap)
    assert st["flagged"] > 0 and st["patterns"] == len(pats) and st["bases"] == sum(len(p) for p in pats)
    if seg_len < 4096:
        assert mm.odd_starts(pats, want, rig.n, seg_len, overlap) >= 1
    rig.check(pats[::-1], seg_len, overlap, want[::-1])


@pytest.mark.parametrize("seg_len,overlap", mm.SETTINGS)
def test_random_patterns(rig, random_want, seg_len, overlap):
    """(a): no match reaches across an overlap of 16 (the oracle's lengths say so), so nothing is flagged there"""
    pats, want = random_want
    st, (tab, flags, runs), _ = rig.check(pats, seg_len, overlap, want)
    if overlap >= 16:
        assert max(int(w[1].max()) for w in want) <= 16 and not any(flags)
        assert st["flagged"] == 0 and st["chain_runs"] == 0 and st["steps_chain"] == 0


@pytest.mark.parametrize("seg_len,overlap", mm.SETTINGS)
def test_substring_is_one_chain(rig, medium_case, seg_len, overlap):
    """(b): every segment but the last is flagged and one lane walks them all"""
    st, _, _ = rig.check([mm.substring_pattern(medium_case, seg_len)], seg_len, overlap)
    assert st["segments"] >= 10 and st["flagged"] == st["segments"] - 1 and st["chain_runs"] == 1


@pytest.mark.parametrize("seg_len,overlap", mm.SETTINGS)
def test_haplotype_is_mixed(rig, medium_case, seg_len, overlap):
    """(c): a whole haplotype with a substitution every ~300 bases.  With an overlap of 0 a segment is flagged as soon as its last base occurs in the
    text at all, so every segment but the last is, and they are one run; the mixed outcome is asserted where the overlap can tell (16 and more)."""
    st, _, _ = rig.check([mm.haplotype_pattern(medium_case)], seg_len, overlap)
    assert 0 < st["flagged"] < st["segments"]
    if overlap >= 16:
        assert st["chain_runs"] > 1
    if overlap == 0:
        assert st["flagged"] == st["segments"] - 1 and st["chain_runs"] == 1


def test_uncut_equals_ms_lengths_batch(rig, medium_case):
    """seg_len >= the longest pattern: pointers and lengths are moni_ms_lengths_batch's exactly; and either output alone is the same output"""
    pats = mm.ragged_batch(medium_case, 64, 16)
    seq, offs = mm.ragged(pats)
    ptr0, ln0 = rig.ctx.ms_lengths_batch(seq, offs)
    ptr, ln, st = rig.ctx.ms_long_batch(seq, offs, 1 << 20, 256)
    assert np.array_equal(ptr, ptr0) and np.array_equal(ln, ln0)
    assert st["segments"] == sum(1 for p in pats if p) and st["flagged"] == 0 and st["steps_spec"] == len(seq)
    ptr1, ln1, _ = rig.ctx.ms_long_batch(seq, offs, 64, 16)
    assert np.array_equal(ln1, ln0)
    only_p, none_l, _ = rig.ctx.ms_long_batch(seq, offs, 64, 16, want_lengths=False)
    none_p, only_l, _ = rig.ctx.ms_long_batch(seq, offs, 64, 16, want_pointers=False)
    assert none_l is None and none_p is None and np.array_equal(only_p, ptr1) and np.array_equal(only_l, ln1)
    assert rig.ctx.kernel_ms(0) > 0 and rig.ctx.kernel_ms(1) > 0 and rig.ctx.kernel_ms(2) >= 0


def test_arguments_and_resident_batch(rig, medium_case):
    from moni_align_amd import capi
    L = rig.ctx._L
    pats = [medium_case.text[100:400], b"", medium_case.text[5000:5100]]
    seq, offs = mm.ragged(pats)
    b, keep = rig.ctx._batch(seq, offs)
    out = np.zeros(len(seq), dtype=np.uint64)
    p = capi.MslongParamsC()
    L.moni_mslong_params_default(ctypes.byref(p))
    call = lambda prm, a, c: L.moni_ms_long_batch(rig.ctx._h, ctypes.byref(b), ctypes.byref(prm) if prm is not None else None, a, c, None)
    assert call(p, out.ctypes.data, None) == 0 and int(out[0]) < rig.n          # stats may be NULL
    assert call(p, None, None) == -22 and call(None, out.ctypes.data, None) == -22
    p.seg_len = 7
    assert call(p, out.ctypes.data, None) == -22
    p.seg_len = 8
    p.reserved[1] = 1
    assert call(p, out.ctypes.data, None) == -22
    # empty batch, empty patterns
    e_ptr, e_ln, st = rig.ctx.ms_long_batch(np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    assert len(e_ptr) == 0 and st["segments"] == 0 and st["patterns"] == 0
    e_ptr, e_ln, st = rig.ctx.ms_long_batch(np.zeros(0, np.uint8), np.zeros(4, np.uint64))
    assert len(e_ln) == 0 and st["segments"] == 0 and st["patterns"] == 3
    # the call leaves no batch the other entry points could run on
    rig.ctx.ms_long_batch(seq, offs)
    with pytest.raises(RuntimeError):
        rig.ctx.pml_run(25)
    with pytest.raises(RuntimeError):
        rig.ctx.ms_run()
    ptr0, ln0 = rig.ctx.ms_lengths_batch(seq, offs)                              # and the next upload works as ever
    assert int(ln0[0]) == 300


def test_long_runs_and_cold_letters(tmp_path):
    """(e): runs past the 12-bit length field, a letter without a hot slot (N occurs in this BWT), the general path"""
    from tests.test_host_sim import long_run_case
    fi, reads = long_run_case()
    path = str(tmp_path / "long_runs.mfi")
    fi.save(path)
    text = fi.text.tobytes()
    pats = [r.tobytes() for r in reads[:60]]
    rng = np.random.default_rng(21)
    for at, L in ((500, 9000), (33000 - 20, 5000), (100000, 12001)):
        w = np.frombuffer(text[at:at + L], dtype=np.uint8).copy()
        for e in rng.integers(0, L, size=L // 700):
            w[int(e)] = mm.ACGT[int(rng.integers(0, 4))]
        pats.append(w.tobytes())
    r = Rig(fi, path)
    try:
        want = [r.orc.ms_lengths(p) for p in pats]
        for seg_len, overlap in mm.SETTINGS:
            st, _, _ = r.check(pats, seg_len, overlap, want)
            assert st["jumps"] > 0
        assert max(int(w[1].max()) for w in want) >= 150
    finally:
        r.close()


def test_cli_split(medium_case, tmp_path):
    import __graft_entry__
    __graft_entry__.build()
    rng = np.random.default_rng(31)
    pats = [mm.mutate(medium_case.pg.seqs[5][:30011], rng).tobytes(), medium_case.text[700:1900], b"ACGTNNNNACGT" * 9,
            mm.mutate(medium_case.pg.seqs[0][40000:52000], rng).tobytes()]
    fa = str(tmp_path / "pats.fa")
    with open(fa, "wb") as f:
        for i, p in enumerate(pats):
            f.write(b">chr%d\n" % i + p + b"\n")
    outs = {}
    for mode in ("--ms", "--mems"):
        for tag, extra in (("plain", []), ("split", ["--split", "--seg-len", "512", "--overlap", "64"])):
            out = str(tmp_path / (mode[2:] + "_" + tag))
            r = subprocess.run([EXE, medium_case.path[:-4], "-p", fa, "-o", out, mode, "-t", "2"] + extra, capture_output=True)
            assert r.returncode == 0, r.stderr
            outs[(mode, tag)] = out
    assert open(outs[("--ms", "split")] + ".lengths", "rb").read() == open(outs[("--ms", "plain")] + ".lengths", "rb").read()
    assert open(outs[("--mems", "split")] + ".mems", "rb").read() == open(outs[("--mems", "plain")] + ".mems", "rb").read()
    lens = open(outs[("--ms", "split")] + ".lengths", "rb").read().split(b"\n")
    assert lens[0] == b">chr0" and len(lens[1].split()) == len(pats[0])
    # the pointers of the split run name positions where the text holds the match
    ptrs = open(outs[("--ms", "split")] + ".pointers", "rb").read().split(b"\n")
    q, l = [int(x) for x in ptrs[3].split()], [int(x) for x in lens[3].split()]
    assert len(q) == len(pats[1]) == 1200 and l[0] == 1200 and medium_case.text[q[0]:q[0] + 1200] == pats[1]
