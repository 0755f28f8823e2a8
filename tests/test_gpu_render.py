"""finish_render_kernel spells a SAM line from the recipe finish_prep_kernel leaves: the line is laid out with one lane per segment, every literal, number
and sequence name is written by the lane that owns it, and the long pieces (the read's name, SEQ, QUAL, the CIGARs, MD) by all lanes together.  The bytes
must not show any of that: the SAM text of moni_align_run equals the oracle's byte for byte, on batches built for the places where the layout takes another
path: unaligned records and
records without qualities; lines around the 1280 bytes of the LDS staging; sequence names read from HBM (more than AFW_NAMES = 1024 bytes of them, more than
AFW_NSEQ = 126 sequences); no ZS tag; deletion items in MD; and more alternatives than one pass of the lanes holds segments for (36 + 6 per alternative > 64).
Every test asserts on the oracle's own text that its batch holds the case it is there for."""
import numpy as np
import pytest

from tests.test_gpu_align import first_diff
from tests.test_gpu_prep_tail import _arrays, _mixed_batch, _sub

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


class Case:
    """an index of given sequences (unrelated: no lifts), the oracle's handle and a GPU context on it"""

    def __init__(self, tmp_path, seqs, names):
        from moni_align_amd import capi, index_build, synth
        from oracle import orc
        self.pg = synth.Pangenome(seqs=seqs, names=names, w=10)
        self.fi = index_build.build_from_pangenome(self.pg, device="cpu")
        path = str(tmp_path / "case.mfi")
        self.fi.save(path)
        self.oracle = orc.OracleIndex(path)
        self.idx = capi.Index(fi=self.fi)
        self.ctx = capi.Ctx(self.idx)

    def close(self):
        self.ctx.close()
        self.idx.close()


def related_seqs(n, length, n_sub, seed):
    """n sequences: a random one and copies of it with n_sub substituted bases each"""
    rng = np.random.default_rng(seed)
    base = ACGT[rng.integers(0, 4, size=length)]
    return [base] + [_sub(base, [int(x) for x in rng.choice(length, size=n_sub, replace=False)]) for _ in range(n - 1)]


def sampled_reads(seqs, n, lo, hi, max_sub, seed):
    """n reads of lo .. hi bases from random places of random sequences, 0 .. max_sub substituted bases each, both strands"""
    from moni_align_amd import synth
    rng = np.random.default_rng(seed)
    reads = []
    for _ in range(n):
        s = seqs[int(rng.integers(0, len(seqs)))]
        m = int(rng.integers(lo, hi + 1))
        p = int(rng.integers(0, len(s) - m + 1))
        r = _sub(s[p:p + m], [int(x) for x in rng.integers(0, m, size=int(rng.integers(0, max_sub + 1)))])
        reads.append(r if rng.random() < 0.5 else synth.revcomp(r[None, :])[0].copy())
    return reads


def run(ctx, arr, quals=True):
    seq, offs, names, noff, q = arr
    ctx.upload(seq, offs)
    return ctx.align_run(names, noff, q if quals else None, host_threads=8)


def same(got, want):
    if got != want:
        raise AssertionError("SAM differs at record %d:\n got: %s\nwant: %s" % first_diff(got, want))


def oracle_text(oracle, arr, quals=True):
    from oracle import orc
    seq, offs, names, noff, q = arr
    return orc.align_batch(oracle, seq, offs, names, noff, q if quals else None, threads=8)[0]


def tag(line, key):
    for f in line.split(b"\t")[11:]:
        if f.startswith(key):
            return f[len(key):]
    return None


def n_alternatives(line):
    aa = tag(line, b"AA:Z:")
    return 0 if aa is None else aa.count(b";")


@pytest.fixture(scope="module")
def medium_env(medium_case):
    from moni_align_amd import capi
    from oracle import orc
    idx = capi.Index(fi=medium_case.fi)
    ctx = capi.Ctx(idx)
    yield orc.OracleIndex(medium_case.path), ctx, _arrays(_mixed_batch(medium_case))
    ctx.close()
    idx.close()


@pytest.mark.parametrize("quals", [True, False])
def test_mixed_batch_equals_the_oracle(medium_env, quals):
    oracle, ctx, arr = medium_env
    want = oracle_text(oracle, arr, quals)
    lines = want.split(b"\n")[:-1]
    flags = [int(l.split(b"\t")[1]) for l in lines]
    assert 0 in flags and 16 in flags and 4 in flags                                    # both strands, unaligned records
    cig = [l.split(b"\t")[5] for l in lines]
    assert any(b"I" in c for c in cig) and any(b"D" in c for c in cig) and any(b"^" in (tag(l, b"MD:Z:") or b"") for l in lines)
    assert all((l.split(b"\t")[10] == b"*") != quals for l in lines)
    got, st = run(ctx, arr, quals)
    same(got, want)


def test_lines_around_the_capacity_of_the_staging(tmp_path):
    """14 related sequences with names of 90 characters (1260 bytes of names: they are read from HBM) and reads of 430 to 512 bases: lines of 1265 to 1280
    bytes, the newline included, are spelled by the kernel up to the staging's last byte; a line of 1281 or more goes to the host pipeline and is counted"""
    names = [("sequence_%02d_" % k) + "n" * 78 for k in range(14)]
    assert all(len(x) == 90 for x in names)
    c = Case(tmp_path, related_seqs(14, 6000, 12, seed=5), names)
    try:
        arr = _arrays(sampled_reads(c.pg.seqs, 600, 430, 512, 11, seed=5))
        want = oracle_text(c.oracle, arr)
        lens = np.array([len(l) + 1 for l in want.split(b"\n")[:-1]])
        assert ((lens >= 1265) & (lens <= 1280)).sum() >= 1 and (lens == 1280).sum() >= 1 and ((lens >= 1281) & (lens <= 1296)).sum() >= 1, \
            (int(lens.max()), int(((lens >= 1265) & (lens <= 1280)).sum()), int((lens == 1280).sum()), int(((lens >= 1281) & (lens <= 1296)).sum()))
        got, st = run(c.ctx, arr)
        same(got, want)
        assert st["handover_why"].get("capacity", 0) >= 1, st
    finally:
        c.close()


def test_more_sequences_than_the_name_table_holds(tmp_path):
    """130 unrelated sequences: no second chain, so no record has ZS; noisy reads with deletions: ^ items in MD"""
    rng = np.random.default_rng(9)
    seqs = [ACGT[rng.integers(0, 4, size=1500)] for _ in range(130)]
    c = Case(tmp_path, seqs, ["u%d" % k for k in range(130)])
    try:
        from moni_align_amd import synth
        arr = _arrays(list(synth.make_reads(c.pg, 600, 150, seed=31, sub_rate=0.02, indel_rate=0.004)))
        want = oracle_text(c.oracle, arr)
        lines = want.split(b"\n")[:-1]
        aligned = [l for l in lines if int(l.split(b"\t")[1]) != 4]
        assert len(aligned) >= 500 and not any(tag(l, b"ZS:i:") is not None for l in lines)
        assert sum(1 for l in aligned if b"^" in tag(l, b"MD:Z:")) >= 50
        got, st = run(c.ctx, arr)
        same(got, want)
    finally:
        c.close()


def repeat_case(tmp_path, n_sub, seed, read_len=100):
    """one sequence: 400-base segments in 6, 8, 10, 12 and 16 copies, n_sub substituted bases per copy, random bases between the copies; 40 reads of 100
    bases per segment, 2 substituted bases each, both strands"""
    from moni_align_amd import synth
    rng = np.random.default_rng(seed)
    parts, copies = [], []
    for n_copy in (6, 8, 10, 12, 16):
        seg = ACGT[rng.integers(0, 4, size=400)]
        mine = [_sub(seg, [int(x) for x in rng.choice(400, size=n_sub, replace=False)]) for _ in range(n_copy)]
        copies.append(mine)
        for x in mine:
            parts += [x, ACGT[rng.integers(0, 4, size=300)]]
    order = rng.permutation(len(parts) // 2)
    seq = np.concatenate([np.concatenate([parts[2 * k], parts[2 * k + 1]]) for k in order])
    reads = []
    for mine in copies:
        for _ in range(40):
            x = mine[int(rng.integers(0, len(mine)))]
            p = int(rng.integers(0, 400 - read_len))
            r = _sub(x[p:p + read_len], [int(v) for v in rng.choice(read_len, size=2, replace=False)])
            reads.append(r if rng.random() < 0.5 else synth.revcomp(r[None, :])[0].copy())
    return Case(tmp_path, [seq], ["rep"]), _arrays(reads)


def test_more_alternatives_than_a_wavefront_has_lanes_for(tmp_path):
    """five alternatives are 66 segments: the layout takes a second pass of the lanes"""
    c, arr = repeat_case(tmp_path, 4, seed=17)
    try:
        want = oracle_text(c.oracle, arr)
        n_alt = np.array([n_alternatives(l) for l in want.split(b"\n")[:-1]])
        many = int((n_alt >= 5).sum())
        assert len(n_alt) == 200 and many >= 10 and n_alt.max() <= 16, (many, int(n_alt.max()))          # (16 = AF_MAX_CAND: the recipe holds them all)
        got, st = run(c.ctx, arr)
        same(got, want)
        assert st["handed_back"] + st["kernel_fallback"] < many, st
    finally:
        c.close()


def test_more_alternatives_than_the_recipe_holds(tmp_path):
    """copies that differ less give more alternatives than the recipe has room for (AF_MAX_CAND = 16): whoever spells these lines, the text is the oracle's"""
    c, arr = repeat_case(tmp_path, 2, seed=17)
    try:
        want = oracle_text(c.oracle, arr)
        assert max(n_alternatives(l) for l in want.split(b"\n")[:-1]) > 16
        got, _ = run(c.ctx, arr)
        same(got, want)
    finally:
        c.close()
