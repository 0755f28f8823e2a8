"""Occurrence lists used in place: the count pass of the seeding stage leaves every seed's list where it wrote it (16 entries per MEM slot), a seed
that keeps more gets bump-allocated space in an overflow region behind them and is walked again by a second, small launch, and the align paths
read the lists through occ_off / occ_cnt alone; moni_seed_fetch compacts on demand.  The index here is a synthetic text with planted identical
copies, so that chosen seeds occur exactly 15, 16, 17 and 40 times: both sides of the in-place cap.  Parity checks: no tolerance."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 16                       # entries per MEM slot (moni_ctx::tmp_cap)
COPIES = (15, 16, 17, 40)      # occurrences of the planted units
UNIT = 200


class Planted:
    """three unrelated sequences of 30 kb; unit k (200 random bases) is written COPIES[k] times at places 400 apart, dealt over the sequences"""

    def __init__(self, tmpdir):
        from moni_align_amd import index_build, synth
        from oracle import orc
        rng = np.random.default_rng(4242)
        acgt = np.frombuffer(b"ACGT", np.uint8)
        seqs = [acgt[rng.integers(0, 4, size=30000)] for _ in range(3)]
        places = [(s, p) for s in range(3) for p in range(200, 29600, 400)]
        order = rng.permutation(len(places))
        self.where = []            # per unit: its (sequence, position) copies
        at = 0
        for k in COPIES:
            unit = acgt[rng.integers(0, 4, size=UNIT)]
            here = [places[i] for i in order[at:at + k]]
            at += k
            for s, p in here:
                seqs[s][p:p + UNIT] = unit
            self.where.append(here)
        self.free = [places[i] for i in order[at:]]          # places that hold no copy: unique text
        self.pg = synth.Pangenome(seqs=seqs, names=["a", "b", "c"], w=10, variants=None)
        self.fi = index_build.build_from_pangenome(self.pg, device="cpu")
        self.path = os.path.join(str(tmpdir), "planted.mfi")
        self.fi.save(self.path)
        self.oidx = orc.OracleIndex(self.path)
        self.synth = synth

    def reads(self, units, n, seed, L=150, spill=True):
        """n reads of L bases over copies of the given units (None: over unique text), half of them reverse-complemented.  spill: a third of them start
        up to 60 bases before the unit or end up to 60 behind it, so that shorter MEMs with the unit's count stand beside unique ones"""
        rng = np.random.default_rng(seed)
        out = []
        for _ in range(n):
            here = self.free if units is None else self.where[units[int(rng.integers(0, len(units)))]]
            s, p = here[int(rng.integers(0, len(here)))]
            lo = int(rng.integers(0, UNIT - L + 1))
            if spill and rng.random() < 1 / 3:
                lo = int(rng.integers(-60, 0)) if rng.random() < 0.5 else int(rng.integers(UNIT - L + 1, UNIT - L + 61))
            r = self.pg.seqs[s][p + lo:p + lo + L].copy()
            out.append(self.synth.revcomp(r[None, :])[0].copy() if rng.random() < 0.5 else r)
        return out


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    return Planted(tmp_path_factory.mktemp("planted"))


@pytest.fixture(scope="module")
def gpu(planted):
    from moni_align_amd import capi
    idx = capi.Index(fi=planted.fi)
    yield idx
    idx.close()


def ragged(reads):
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate(reads), offs


def seeds_on_gpu(ctx, seq, offs, **kw):
    ctx.upload(seq, offs)
    ctx.seed_run(25, kw.get("filter_seeds", True), kw.get("n_seeds_thr", 1000))
    got = ctx.seed_fetch()
    got["counters"] = ctx.counters()
    return got, ctx.seed_occ_stats()


def sam_both(planted, ctx, seq, offs):
    from oracle import orc
    from tests.test_gpu_align import first_diff
    names, noff = orc.make_names(len(offs) - 1)
    q = np.full(len(seq), ord("I"), dtype=np.uint8)
    want, wcnt = orc.align_batch(planted.oidx, seq, offs, names, noff, q, threads=8)
    got, st = ctx.align_batch(seq, offs, names, noff, q, host_threads=8)
    if got != want:
        raise AssertionError("SAM differs at record %d:\n got: %s\nwant: %s" % first_diff(got, want))
    assert st["aligned"] == wcnt["aligned"]
    return got, st


@pytest.fixture(scope="module")
def boundary_batch(planted):
    """400 reads over all four units: lists of 15 and 16 stay in their slots, lists of 17 and 40 go to the overflow region; every read is long enough
    (>= 2 x min_len) for its MEM to be split, so the left halves take the same two ways.  The oracle's seeds of the batch, computed once."""
    seq, offs = ragged(planted.reads([0, 1, 2, 3], 400, seed=1))
    want = planted.oidx.seed_batch(seq, offs, 25, True, 1000, threads=4)
    return seq, offs, want


def test_boundary_of_the_in_place_cap(planted, gpu, boundary_batch):
    from moni_align_amd import capi
    from tests.parity import assert_seeds_equal
    seq, offs, want = boundary_batch
    cnt = want["occ_cnt"]
    for k in COPIES:                                        # the planted counts are what the seeds have, on both sides of the cap
        assert int((cnt == k).sum()) > 50, (k, np.unique(cnt))
    assert len(cnt) >= 3 * 400                              # a MEM and its two halves per read: every MEM here is long enough to be split
    ctx = capi.Ctx(gpu)
    try:
        got, st = seeds_on_gpu(ctx, seq, offs)
        assert_seeds_equal(got, want)
        assert np.array_equal(got["counters"], want["counters"])
        n_long = int((cnt > CAP).sum())
        assert st["long_seeds"] == n_long and st["overflow_used"] == int(cnt[cnt > CAP].sum()) and st["long_launches"] == 1
        assert st["compactions"] == 1                       # the fetch compacted; the align path below does not
        _, ast = sam_both(planted, ctx, seq, offs)
        assert ast["handed_back"] == 0                      # (a read handed to the host pipeline would be seeded again there, with a fetch)
        assert ctx.seed_occ_stats()["compactions"] == 0
    finally:
        ctx.close()


def test_per_genome_filter_with_overflow(planted, gpu):
    """filter_seeds with n_seeds_thr = 6, below every planted count: every planted seed is walked a second time with a row of per-genome counters
    (2000 reads x 3 seeds: more rows than the 4096 a fresh context has, so the count pass is repeated on a larger pool), the seeds with 40 copies
    lose occurrences to the filter and stay long, and some that saw 17 keep 16 or fewer and stay in place.  The oracle's align entry point takes no threshold,
    so against the oracle this case compares the seeds and occurrences (with the filter counts and the work counters); the align kernels over the
    filtered long lists are checked against themselves: the SAM text of a fresh context (pool and region grown inside the call) equals the grown one's."""
    from moni_align_amd import capi
    from tests.parity import assert_seeds_equal
    seq, offs = ragged(planted.reads([0, 1, 2, 3], 2000, seed=2))
    want = planted.oidx.seed_batch(seq, offs, 25, True, 6, threads=4)
    assert int((want["num_filtered"] > 0).sum()) > 100
    assert int(((want["total_occ"] > CAP) & (want["occ_cnt"] <= CAP)).sum()) > 0 and int(((want["occ_cnt"] > CAP) & (want["num_filtered"] > 0)).sum()) > 0
    assert int((want["total_occ"] > 6).sum()) > 4096
    ctx = capi.Ctx(gpu)
    try:
        got, st = seeds_on_gpu(ctx, seq, offs, n_seeds_thr=6)
        assert_seeds_equal(got, want)
        assert np.array_equal(got["counters"], want["counters"])
        assert st["count_passes"] >= 2 and st["long_seeds"] == int((want["occ_cnt"] > CAP).sum())
        got2, st2 = seeds_on_gpu(ctx, seq, offs, n_seeds_thr=6)          # the grown context: one pass, the same seeds
        assert st2["count_passes"] == 1
        assert_seeds_equal(got2, want)
    finally:
        ctx.close()
    from oracle import orc
    names, noff = orc.make_names(len(offs) - 1)
    ctx = capi.Ctx(gpu)
    try:
        sam1, a1 = ctx.align_batch(seq, offs, names, noff, None, host_threads=8, n_seeds_thr=6)
        sam2, a2 = ctx.align_batch(seq, offs, names, noff, None, host_threads=8, n_seeds_thr=6)
        assert sam1 == sam2 and a1["aligned"] == a2["aligned"] > 0
    finally:
        ctx.close()


def test_overflow_region_growth(planted, gpu, boundary_batch):
    """a fresh context's overflow region holds 4096 entries; the batch's long lists take more, so the first run repeats the count pass on a larger
    array.  Its seeds and its SAM text equal those of a second run on the grown context (one pass), and the oracle's."""
    from moni_align_amd import capi
    from tests.parity import assert_seeds_equal
    seq, offs, want = boundary_batch
    need = int(want["occ_cnt"][want["occ_cnt"] > CAP].sum())
    assert need > 4096
    ctx = capi.Ctx(gpu)
    try:
        got1, st1 = seeds_on_gpu(ctx, seq, offs)
        assert st1["count_passes"] == 2 and st1["overflow_cap"] >= need == st1["overflow_used"]
        got2, st2 = seeds_on_gpu(ctx, seq, offs)
        assert st2["count_passes"] == 1 and st2["overflow_cap"] == st1["overflow_cap"]
        for k in ("mems", "occs", "read_mem_off", "counters"):
            assert np.array_equal(got1[k], got2[k]), k
        assert_seeds_equal(got1, want)
    finally:
        ctx.close()
    ctx = capi.Ctx(gpu)                                     # the align path on a fresh context grows the region the same way
    try:
        sam1, _ = sam_both(planted, ctx, seq, offs)
        assert ctx.seed_occ_stats()["count_passes"] == 2
        sam2, _ = sam_both(planted, ctx, seq, offs)
        assert ctx.seed_occ_stats()["count_passes"] == 1 and sam1 == sam2
    finally:
        ctx.close()


def test_no_long_seeds_skips_the_second_launch(planted, gpu):
    """reads over the units with 15 and 16 copies and over unique text: the longest list fills its slot exactly, none is long, and the long-seed
    kernel is not launched (moni_seed_occ_stats counts its launches)."""
    from moni_align_amd import capi
    from tests.parity import assert_seeds_equal
    seq, offs = ragged(planted.reads([0, 1], 200, seed=3) + planted.reads(None, 100, seed=4))
    want = planted.oidx.seed_batch(seq, offs, 25, True, 1000, threads=4)
    assert int(want["occ_cnt"].max()) == CAP
    ctx = capi.Ctx(gpu)
    try:
        got, st = seeds_on_gpu(ctx, seq, offs)
        assert st["long_launches"] == 0 and st["long_seeds"] == 0 and st["overflow_used"] == 0 and st["count_passes"] == 1
        assert_seeds_equal(got, want)
        assert np.array_equal(got["counters"], want["counters"])
        _, ast = sam_both(planted, ctx, seq, offs)
        assert ast["handed_back"] == 0
        assert ctx.seed_occ_stats()["long_launches"] == 0 and ctx.seed_occ_stats()["compactions"] == 0
    finally:
        ctx.close()


def test_paired_path(planted, gpu):
    """the paired path runs the same seeding stage: pairs drawn over the planted text (mates in and out of the copies), against the paired oracle"""
    from moni_align_amd import capi
    from tests.test_gpu_pe import gpu_align_all
    from tests.test_host_sim_pe import first_diff, interleave, oracle_pe
    from tests.test_oracle_pe import make_pairs
    m1, m2, _ = make_pairs(planted.pg, 600, seed=9)
    want, st = oracle_pe(planted.oidx, m1, m2, b_size=512)
    seq, offs, names, noff, q = interleave(m1, m2)
    ctx = capi.Ctx(gpu)
    try:
        got, model, aligned = gpu_align_all(ctx, seq, offs, names, noff, q, 512)
        assert ctx.seed_occ_stats()["long_seeds"] > 0
    finally:
        ctx.close()
    assert model.count == st["ins_count"] and model.mean == st["ins_mean"] and model.std_dev == st["ins_std_dev"]
    if got != want:
        raise AssertionError("SAM differs at record %d:\n got: %s\nwant: %s" % first_diff(got, want))
    assert aligned == st["aligned"]


def test_extend_path(planted, gpu):
    """extend mode on the same index and reads, against its model.  It seeds with its own longest-MEM search and never runs the occurrence stage, so this
    is a regression run over the repeat-rich text, not a check of the in-place lists."""
    from moni_align_amd import capi
    from tests import extend_model
    reads = [r.tobytes() for r in planted.reads([0, 1, 2, 3], 120, seed=5, L=100)]
    names = [b"x.%d" % i for i in range(len(reads))]
    want, wst = extend_model.extend_batch(planted.oidx, planted.fi, reads, names, None)
    seq, offs = ragged([np.frombuffer(r, np.uint8) for r in reads])
    nm, noff = ragged([np.frombuffer(x, np.uint8) for x in names])
    ctx = capi.Ctx(gpu)
    try:
        got, st = ctx.extend_batch(seq, offs, nm, noff, None)
    finally:
        ctx.close()
    assert got == want and (st["reads"], st["extended"], st["records"]) == (wst["reads"], wst["extended"], wst["records"])
