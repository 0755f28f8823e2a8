"""The result stores of the two seeding walks, on the GPU against the oracle, no tolerance anywhere.
ms_lf_kernel (seed_core.h: ms_task): over the live list of the strand prefilter a task whose sister strand was skipped stores 16 bytes over both
tasks' words, so that a wave writes whole lines; without a list every task stores its own 8.  Read lengths around the 8-step pattern word and the
64-step edges in one batch, ordered so that neighbouring lanes end at different steps, batch sizes at the edges of the 64-task workspace blocks and
the 256-lane thread blocks, a read with a depth of its own, bytes outside A / C / G / T, a stale workspace, the filtered stage with reads that keep
both strands, one or none, an unfiltered walk behind it, and the interleaved variants.  occ_kernel stages the kept occurrences of a seed eight at a
time in LDS: seeds that keep 1, 8, 9, 15, 16, 17 and 40 occurrences (none keeps 0: the first occurrence of a seed is always kept), the per-genome
second walk, the long lists' second launch."""
import os

import numpy as np
import pytest

from tests.parity import assert_seeds_equal
from tests.test_host_ms_stage import COMPL, LENS, length_mix, ragged

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_pair(medium_case):
    from moni_align_amd import capi
    from oracle import orc
    idx = capi.Index(fi=medium_case.fi)
    ctx = capi.Ctx(idx)
    yield orc.OracleIndex(medium_case.path), ctx, idx
    ctx.close()
    idx.close()


def oracle_pointers(o, reads):
    return [np.concatenate([o.ms_query(r.tobytes()), o.ms_query(COMPL[r[::-1]].tobytes())]) for r in reads]


@pytest.fixture(scope="module")
def mix(medium_case, gpu_pair):
    """257 reads of mixed lengths and the oracle's pointers of each, computed once; a batch of n reads is the first n of them"""
    reads = length_mix(medium_case, 257, seed=23)
    assert {len(r) for r in reads} == set(LENS)
    return reads, oracle_pointers(gpu_pair[0], reads)


@pytest.mark.parametrize("n", [1, 31, 33, 257])
def test_pointers_of_mixed_lengths(gpu_pair, mix, n):
    _, ctx, _ = gpu_pair
    reads, want = mix
    assert np.array_equal(ctx.ms_query_batch(*ragged(reads[:n])), np.concatenate(want[:n]))


def test_one_long_read_among_short_ones(medium_case, gpu_pair):
    o, ctx, _ = gpu_pair
    reads = list(medium_case.synth.make_reads(medium_case.pg, 100, 150, seed=29))
    reads[45] = np.frombuffer(bytes(medium_case.fi.text[5000:7000]), dtype=np.uint8).copy()
    assert np.array_equal(ctx.ms_query_batch(*ragged(reads)), np.concatenate(oracle_pointers(o, reads)))


def test_bytes_outside_acgt(medium_case, gpu_pair):
    """the walk writes sample 0 at such a byte: at the first step of a pattern word, at its last, behind it and at the task's last step, on either strand"""
    o, ctx, _ = gpu_pair
    base = medium_case.synth.make_reads(medium_case.pg, 12, 150, seed=31)
    reads = []
    for i, at in enumerate((0, 7, 8, 149, 142, 141)):          # position p is step 149 - p of strand 0 and step p of strand 1
        for j, byte in enumerate((ord("N"), 0x80 + i)):
            r = base[2 * i + j].copy()
            r[at] = byte
            reads.append(r)
    assert np.array_equal(ctx.ms_query_batch(*ragged(reads)), np.concatenate(oracle_pointers(o, reads)))


def test_stale_workspace(medium_case, gpu_pair, mix):
    """long reads, then short ones in the same context: the short batch's words lie where the long batch's were"""
    o, ctx, _ = gpu_pair
    long_reads = [np.frombuffer(bytes(medium_case.fi.text[a:a + 700]), dtype=np.uint8).copy() for a in range(1000, 41000, 1000)]
    ctx.ms_query_batch(*ragged(long_reads))
    reads, want = mix
    assert np.array_equal(ctx.ms_query_batch(*ragged(reads[:70])), np.concatenate(want[:70]))


def test_filtered_stage(medium_case, gpu_pair, mix):
    """what the benchmark runs: the walk over the live list of the strand prefilter, 16-byte stores for the tasks without their sister strand (the
    mixed lengths and the bytes outside A / C / G / T keep both strands of some reads); an unfiltered walk behind it finds every pointer"""
    o, ctx, _ = gpu_pair
    reads = list(medium_case.synth.make_reads(medium_case.pg, 1500, 150, seed=37)) + mix[0]
    seq, offs = ragged(reads)
    want = o.seed_batch(seq, offs, 25, True, 1000, threads=4)
    got = []
    for mode in (2, 0):
        ctx.seed_prefilter(mode)
        ctx.upload(seq, offs)
        ctx.seed_run(25, True, 1000)
        got.append(ctx.seed_fetch())
        if mode == 2:
            assert ctx.seed_prefilter_stats()["skipped"] > 0
            part = reads[-300:]
            assert np.array_equal(ctx.ms_query_batch(*ragged(part)), np.concatenate(oracle_pointers(o, part[:43]) + mix[1]))
    ctx.seed_prefilter(1)
    for g in got:
        assert_seeds_equal(g, want)
    assert got[0]["mems"].tobytes() == got[1]["mems"].tobytes() and np.array_equal(got[0]["occs"], got[1]["occs"])


def test_variants_give_the_same_pointers(medium_case, gpu_pair, mix):
    """MONI_MS_VARIANT (read when a context is made): 1 is the default at another occupancy, 2, 3 and 5 interleave two and four tasks per lane"""
    from moni_align_amd import capi
    _, _, idx = gpu_pair
    reads = mix[0] + list(medium_case.synth.make_reads(medium_case.pg, 43, 150, seed=41))
    want = np.concatenate(mix[1] + oracle_pointers(gpu_pair[0], reads[257:]))
    seq, offs = ragged(reads)
    old = os.environ.get("MONI_MS_VARIANT")
    try:
        for v in (1, 2, 3, 5):
            os.environ["MONI_MS_VARIANT"] = str(v)
            ctx = capi.Ctx(idx)
            try:
                assert np.array_equal(ctx.ms_query_batch(seq, offs), want), v
            finally:
                ctx.close()
    finally:
        if old is None:
            del os.environ["MONI_MS_VARIANT"]
        else:
            os.environ["MONI_MS_VARIANT"] = old


# ---- occ_kernel ----------------------------------------------------------------------------------------------------------------------------
COPIES = (8, 9, 15, 16, 17, 40)


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """the planted text of the in-place occurrence lists' tests, with units that occur 8, 9, 15, 16, 17 and 40 times; unique text gives the seeds with 1"""
    from tests import test_gpu_occ_inplace as tp
    old = tp.COPIES
    tp.COPIES = COPIES
    try:
        return tp.Planted(tmp_path_factory.mktemp("planted_stage"))
    finally:
        tp.COPIES = old


def test_occurrence_lists_at_every_length_of_the_stage(planted):
    from moni_align_amd import capi
    reads = planted.reads(list(range(len(COPIES))), 360, seed=5) + planted.reads(None, 60, seed=6)
    seq, offs = ragged(reads)
    idx = capi.Index(fi=planted.fi)
    ctx = capi.Ctx(idx)
    try:
        for filter_seeds, thr in ((True, 1000), (True, 6), (False, 1000)):          # thr = 6: the second walk with per-genome counters runs for every planted seed
            want = planted.oidx.seed_batch(seq, offs, 25, filter_seeds, thr, threads=4)
            if thr == 1000:
                cnt = want["occ_cnt"]
                for k in (1,) + COPIES:
                    assert int((cnt == k).sum()) > 20, (k, np.unique(cnt))
            ctx.upload(seq, offs)
            ctx.seed_run(25, filter_seeds, thr)
            got = ctx.seed_fetch()
            got["counters"] = ctx.counters()
            assert_seeds_equal(got, want)
            assert np.array_equal(got["counters"], want["counters"])
            if thr == 1000:
                assert ctx.seed_occ_stats()["long_seeds"] == int((cnt > 16).sum()) > 0          # lists of 17 and 40: walked again by occ_long_kernel
    finally:
        ctx.close()
        idx.close()
