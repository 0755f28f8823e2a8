"""The finish stage beside a hand-over read.  A read the staged kernels cannot finish goes to align_kernel, launched with a full grid on a
stream of its own while finish_prep_kernel and finish_render_kernel write the records of the sub-batch's other reads.  align_kernel lets only
as many lanes ask for a read as the launch has reads (lane 0 of every wavefront first), and only wavefronts that took one add to the
statistics: a full grid asking for one read, and flushing zeros, was a burst of 350 000 atomics on one 128-byte line that held up everything
beside it (profiles/prep_tail).  Which lane takes which read must not show: the SAM text of moni_align_run equals the oracle's byte for byte
with the hand-over read in the first sub-batch and in the last, with every read of a batch handed over (more reads than wavefronts: second
lanes take part) and with none (the launch returns at once)."""
import numpy as np
import pytest

from tests.test_gpu_align import first_diff

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _sub(r, at):
    r = r.copy()
    for a in at:
        r[a] = ACGT[(int(np.nonzero(ACGT == r[a])[0][0]) + 1) % 4] if r[a] in ACGT else ACGT[0]
    return r


def _mixed_batch(case):
    """A few thousand reads: noisy samples (every stitching branch occurs among them: chains of overlapping anchors scored by one global problem,
    left and right extensions, gap problems, 1 x 1 gaps, insertions, zero-length deletions) and reads built for the branches one by one, on both
    strands; reads of the reference contig itself; the first and last bases of sequences; a read with an N; and, 50 reads from the end, a read
    of 600 bases: longer than the staged kernels take, so align_kernel gets it."""
    synth, pg = case.synth, case.pg
    reads = list(synth.make_reads(pg, 1500, 150, seed=201, sub_rate=0.02, indel_rate=0.004)) + \
            list(synth.make_reads(pg, 600, 250, seed=202, sub_rate=0.03, indel_rate=0.002)) + \
            list(synth.make_reads(pg, 400, 100, seed=203))
    rng = np.random.default_rng(41)
    built = []
    for h in (0, 2, len(pg.seqs) - 1):          # the reference contig, a haplotype, the last sequence
        s = pg.seqs[h]
        for _ in range(6):
            p = int(rng.integers(200, len(s) - 400))
            e = s[p:p + 150].copy()
            built += [e,                                                       # one MEM
                      _sub(e, [75]),                                           # two MEMs one mismatch apart: the 1 x 1 gap
                      _sub(e, [4, 145]),                                       # left and right extension
                      _sub(e, [70, 73, 77]),                                   # a gap problem between two anchors
                      np.concatenate([e[:80], ACGT[[1, 3]], e[80:148]]),       # insertion
                      np.concatenate([e[:60], s[p + 61:p + 151]]),             # deletion of one base
                      np.concatenate([e[:90], s[p + 93:p + 153]]),             # deletion of three
                      _sub(np.concatenate([e[:40], ACGT[[2]], e[40:149]]), [100, 101])]
        built += [s[:150].copy(), s[-150:].copy(), _sub(s[:150], [0]), _sub(s[-150:], [149])]          # first and last positions of the sequence
    built += [synth.revcomp(r[None, :])[0].copy() for r in built[::2]]
    n_read = built[1].copy(); n_read[33] = ord("N"); built.append(n_read)
    for r in built:
        reads.insert(int(rng.integers(0, len(reads))), r)
    s = pg.seqs[1]
    long_read = _sub(s[3000:3600], list(range(30, 600, 60)))
    reads.insert(len(reads) - 50, long_read)
    return reads


def _arrays(reads):
    from oracle import orc
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    seq = np.concatenate(reads)
    names, noff = orc.make_names(len(reads))
    return seq, offs, names, noff, np.full(len(seq), ord("I"), dtype=np.uint8)


@pytest.fixture(scope="module")
def env(medium_case):
    from moni_align_amd import capi
    from oracle import orc
    idx = capi.Index(fi=medium_case.fi)
    ctx = capi.Ctx(idx)
    yield orc.OracleIndex(medium_case.path), ctx
    ctx.close()
    idx.close()


@pytest.fixture(scope="module")
def mixed(medium_case, env):
    from oracle import orc
    reads = _mixed_batch(medium_case)
    arr = _arrays(reads)
    want, _ = orc.align_batch(env[0], *arr, threads=8)
    return len(reads), arr, want


def _run(ctx, arr):
    seq, offs, names, noff, q = arr
    ctx.upload(seq, offs)
    return ctx.align_run(names, noff, q, host_threads=8)


@pytest.mark.parametrize("where", ["first", "last"])
def test_hand_over_read_in_the_first_and_in_the_last_sub_batch(env, mixed, monkeypatch, where):
    n, arr, want = mixed
    monkeypatch.setenv("MONI_ALIGN_SUB", str(n - 10) if where == "first" else "1000")          # two sub-batches: the long read (50 from the end) in the first; three: in the last
    got, st = _run(env[1], arr)
    if got != want:
        raise AssertionError("SAM differs at record %d:\n got: %s\nwant: %s" % first_diff(got, want))
    assert st["reads"] == n and st["kernel_fallback"] >= 1 and st["handover_why"].get("long_read", 0) >= 1, st
    cig = [f.split(b",")[3] for l in want.split(b"\n") if l for f in l.split(b"\t") if f.startswith(b"OA:Z:")]
    assert any(b"I" in c for c in cig) and any(b"D" in c for c in cig) and len(cig) > n - 400


def test_every_read_handed_over_and_none(medium_case, env):
    """1100 reads of 520 bases: all of them go to align_kernel, more than its 1024 wavefronts, so lanes 0 and 1 ask for reads; then 500 exact
    reads of 150 bases: nothing is handed over."""
    from oracle import orc
    rng = np.random.default_rng(43)
    reads = []
    for _ in range(1100):
        s = medium_case.pg.seqs[int(rng.integers(0, len(medium_case.pg.seqs)))]
        p = int(rng.integers(0, len(s) - 520))
        r = _sub(s[p:p + 520], [int(x) for x in rng.integers(0, 520, size=5)])
        reads.append(r if rng.random() < 0.5 else medium_case.synth.revcomp(r[None, :])[0].copy())
    arr = _arrays(reads)
    want, _ = orc.align_batch(env[0], *arr, threads=8)
    got, st = _run(env[1], arr)
    if got != want:
        raise AssertionError("SAM differs at record %d:\n got: %s\nwant: %s" % first_diff(got, want))
    assert st["kernel_fallback"] == 1100, st
    arr = _arrays(list(medium_case.synth.make_reads(medium_case.pg, 500, 150, seed=204, sub_rate=0.0, indel_rate=0.0)))
    want, _ = orc.align_batch(env[0], *arr, threads=8)
    got, st = _run(env[1], arr)
    assert got == want and st["kernel_fallback"] == 0, st
