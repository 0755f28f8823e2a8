"""pack_filter_kernel (csrc/packfilter_core.h), the fused front end of the filtered seeding stage, on the GPU against the two kernels it replaces
(a context made with MONI_SEED_FUSE=0): seeds, work counters, filter statistics and SAM text are the same; byte words that an earlier batch left
behind skipped tasks are never read; and a run without the filter that follows a filtered one finds its complete workspace.  On medium_case."""
import numpy as np
import pytest

from tests.test_gpu_strand_skip import COMPL, MIN_LEN, ragged, ragged_reads

pytestmark = pytest.mark.gpu

LENS = (0, 1, 7, 8, 9, 24, 25, 26, 31, 32, 33, 63, 64, 65, 150, 159, 160, 161, 250, 256, 257)


@pytest.fixture(scope="module")
def ctxs(medium_case):
    """one index; a context on the fused path, one on the two kernels, and a way to make more"""
    import os
    from moni_align_amd import capi
    idx = capi.Index(fi=medium_case.fi)
    made = []

    def make(fuse):
        old = os.environ.get("MONI_SEED_FUSE")
        os.environ["MONI_SEED_FUSE"] = "1" if fuse else "0"          # read when the context is created
        try:
            made.append(capi.Ctx(idx))
        finally:
            if old is None:
                del os.environ["MONI_SEED_FUSE"]
            else:
                os.environ["MONI_SEED_FUSE"] = old
        return made[-1]

    yield make(True), make(False), make
    for c in made:
        c.close()
    idx.close()


def length_reads(mc):
    """four reads of every length of LENS: two as sequenced, one with N at both ends and at the 8-byte and 32-base boundaries, one with a lower-case base and a byte >= 0x80"""
    base = mc.synth.make_reads(mc.pg, 4 * len(LENS), 257, seed=31, sub_rate=0.01)
    reads = []
    for i, m in enumerate(LENS):
        for j in range(4):
            r = base[4 * i + j][:m].copy()
            if j == 2:
                for at in (0, 7, 8, 31, 32, m - 1):
                    if 0 <= at < m:
                        r[at] = ord("N")
            if j == 3 and m:
                r[m // 2] |= 0x20
                r[m // 3] = 0x80 + m % 100
            reads.append(r)
    return reads


def seed_state(ctx, seq, offs, mode=2):
    ctx.seed_prefilter(mode)
    ctx.upload(seq, offs)
    ctx.seed_run(MIN_LEN, True, 1000)
    out = ctx.seed_fetch()
    out["counters"] = ctx.counters()
    out["stats"] = ctx.seed_prefilter_stats()
    ctx.seed_prefilter(1)
    return out


def assert_same_seeds(a, b):
    assert np.array_equal(a["read_mem_off"], b["read_mem_off"])
    assert a["mems"].tobytes() == b["mems"].tobytes()
    assert np.array_equal(a["occs"], b["occs"])


def test_seeds_counters_statistics(medium_case, ctxs):
    fused, two, _ = ctxs
    reads = ragged_reads(medium_case) + length_reads(medium_case)
    seq, offs = ragged(reads)
    a, b = seed_state(fused, seq, offs), seed_state(two, seq, offs)
    print("fused %s %s; two kernels %s %s" % (a["stats"], a["counters"], b["stats"], b["counters"]))
    assert_same_seeds(a, b)
    assert np.array_equal(a["counters"], b["counters"])
    assert a["stats"]["tasks"] == b["stats"]["tasks"] == 2 * len(reads)
    assert a["stats"]["skipped"] == b["stats"]["skipped"] > 0
    assert a["stats"]["density"] == b["stats"]["density"]
    assert a["stats"]["lookups"] <= b["stats"]["lookups"]
    assert a["stats"]["lookups"] > 0


def test_sam_single_end(medium_case, ctxs):
    fused, two, _ = ctxs
    reads = list(medium_case.synth.make_reads(medium_case.pg, 3000, 150, seed=88)) + [r for r in length_reads(medium_case) if len(r)]
    seq, offs = ragged(reads)
    names, noff = medium_case.synth.make_names(len(reads))
    quals = np.full(seq.size, ord("I"), dtype=np.uint8)
    sam = []
    for ctx in (fused, two):
        s, _ = ctx.align_batch(seq, offs, names, noff, quals, host_threads=4)
        assert ctx.seed_prefilter_stats()["skipped"] > 0
        sam.append(s)
    assert sam[0] == sam[1]


def test_sam_paired(medium_case, ctxs):
    fused, two, _ = ctxs
    pg, synth = medium_case.pg, medium_case.synth
    rng = np.random.default_rng(17)
    pr = []
    for _ in range(1000):
        sq = pg.seqs[int(rng.integers(0, len(pg.seqs)))]
        ins = int(max(210, rng.normal(350, 30)))
        at = int(rng.integers(0, len(sq) - ins))
        pr.append(sq[at:at + 100].copy())
        pr.append(synth.revcomp(sq[None, at + ins - 100:at + ins])[0].copy())
    seq, offs = ragged(pr)
    pnames = [("p%d/%d" % (i, k + 1)).encode() for i in range(1000) for k in range(2)]
    noff = np.zeros(len(pnames) + 1, np.uint64); noff[1:] = np.cumsum([len(x) for x in pnames])
    names = np.frombuffer(b"".join(pnames), np.uint8)
    quals = np.full(seq.size, ord("I"), np.uint8)
    model = two.pe_learn(seq, offs)
    sam = []
    for ctx in (fused, two):
        s, _ = ctx.pe_align(seq, offs, names, noff, quals, model, host_threads=4)
        assert ctx.seed_prefilter_stats()["skipped"] > 0
        sam.append(s)
    assert sam[0] == sam[1]


def test_stale_byte_words(medium_case, ctxs):
    """batch A, then its reverse complements in the same context: live and skipped tasks swap places over the byte words A left behind"""
    fused, _, make = ctxs
    a_reads = list(medium_case.synth.make_reads(medium_case.pg, 2000, 150, seed=61))
    b_reads = [COMPL[r[::-1]] for r in a_reads]
    seq_a, offs_a = ragged(a_reads)
    seq_b, offs_b = ragged(b_reads)
    names, noff = medium_case.synth.make_names(len(a_reads))
    quals = np.full(seq_a.size, ord("I"), dtype=np.uint8)
    fresh = make(True)
    sa = seed_state(fused, seq_a, offs_a)
    sb = seed_state(fused, seq_b, offs_b)
    want = seed_state(fresh, seq_b, offs_b)
    assert sa["stats"]["skipped"] > 0 and sb["stats"]["skipped"] == want["stats"]["skipped"] > 0
    assert_same_seeds(sb, want)
    assert np.array_equal(sb["counters"], want["counters"])
    fused.align_batch(seq_a, offs_a, names, noff, quals, host_threads=4)
    sam_b, _ = fused.align_batch(seq_b, offs_b, names, noff, quals, host_threads=4)
    want_sam, _ = make(True).align_batch(seq_b, offs_b, names, noff, quals, host_threads=4)
    assert sam_b == want_sam


def test_unfiltered_pointers_after_a_filtered_run(medium_case, ctxs):
    fused, two, _ = ctxs
    reads = list(medium_case.synth.make_reads(medium_case.pg, 500, 150, seed=150))
    seq, offs = ragged(reads)
    want = two.ms_query_batch(seq, offs)
    assert seed_state(fused, seq, offs)["stats"]["skipped"] > 0
    assert np.array_equal(fused.ms_query_batch(seq, offs), want)
