"""The seeding stage over event lists, on the GPU, no tolerance anywhere: ms_lf_events_kernel records the assignments of a walk (seed_core.h:
ms_task_events) and mem_events_kernel rebuilds the pointers from them, where MONI_MS_EVENTS=0 keeps the dense pointers.  Every batch is seeded by a
context of either kind and compared with the oracle's seed_batch and with the other context byte for byte, counters included.  Read lengths 1, 7, 8, 9,
63, 64, 65, 150, 161 (the eight-word instance of the MEM kernels) and 300 (byte comparison), ordered so that neighbouring lanes differ; copies of the
text (short lists), random reads and reverse complements (the wrong strand: long lists); lists of 1, 7, 8, 9, 16 and 17 events, selected from a pool by the
oracle's pointers, so that the stage of eight flushes at every edge; an N and a byte >= 0x80 at the first and the last base and in front of matching bases
(the decrement of 0 wraps); reads with more than MONI_MEM_SLOTS MEMs on a strand (the emit pass walks them again); batches of 1, 31, 33 and 257 reads; the
strand prefilter on and off; a short batch behind a long one; ms_query_batch behind a seeding run; one single-end and one paired batch as SAM text."""
import os

import numpy as np
import pytest

from tests.parity import assert_seeds_equal
from tests.test_host_ms_events import EDGES, event_counts
from tests.test_host_ms_stage import COMPL, ragged

pytestmark = pytest.mark.gpu

LENS = (1, 7, 8, 9, 63, 64, 65, 150, 161, 300)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def oracle_pointers(o, r):
    return np.concatenate([o.ms_query(r.tobytes()), o.ms_query(COMPL[r[::-1]].tobytes())])


def text_copy(text, rng, m):
    while True:
        at = int(rng.integers(100, len(text) - 400))
        r = text[at:at + m].copy()
        if np.isin(r, ACGT).all():
            return r


def chimera(text, rng, n_parts, part):
    """pieces of the text from places of their own: a MEM each"""
    return np.concatenate([text_copy(text, rng, part) for _ in range(n_parts)])


def event_mix(mc, o, seed=11):
    """257 reads and the oracle's pointers of each.  Read i has length LENS[3 i mod 10] and is by turns a copy of the text, a copy with substitutions, a
    random read and the reverse complement of a copy; some of the first are chosen so that lists of every length of EDGES occur among the first 31."""
    rng = np.random.default_rng(seed)
    text = np.frombuffer(bytes(mc.fi.text), dtype=np.uint8)

    def make(i, m):
        kind = i % 4
        if kind == 2:
            return ACGT[rng.integers(0, 4, size=m)]
        r = text_copy(text, rng, m)
        if kind == 1:
            hit = rng.random(m) < 0.04
            r[hit] = ACGT[rng.integers(0, 4, size=int(hit.sum()))]
        return COMPL[r[::-1]].copy() if kind == 3 else r

    reads = [make(i, LENS[(3 * i) % 10]) for i in range(257)]
    special = {3: COMPL[chimera(text, rng, 6, 50)[::-1]].copy(),                                   # six MEMs of 50 (split in halves) on strand 1 of a read that compares bytes
               6: np.concatenate([chimera(text, rng, 5, 32), text_copy(text, rng, 1)]),            # five MEMs on strand 0, 161 bases
               9: chimera(text, rng, 5, 30)}                                                       # ... and 150
    # bytes outside A / C / G / T: first base, last base, and inside a copy of the text, where matching bases follow on either strand
    # (the step behind an absent byte starts from the first suffix of that byte's place in the order: whether it is a match is the index's affair, so
    # the read with an N inside is taken from candidates until the oracle's pointers show the wrapped word; a byte >= 0x80 sorts behind every suffix, and
    # the step behind it always jumps)
    for k, (at, byte) in enumerate(((0, ord("N")), (149, ord("N")), (60, ord("N")), (0, 0x80), (149, 0xC1), (60, 0xFF))):
        for tries in range(400):
            r = text_copy(text, rng, 150)
            r[at] = byte
            if (at, byte) != (60, ord("N")) or (oracle_pointers(o, r) >> np.uint64(40)).any():
                break
        special[19 + 10 * k] = r
    for i, r in special.items():
        assert len(r) == len(reads[i])
        reads[i] = r
    ptrs = [oracle_pointers(o, r) for r in reads]
    # lists of every edge length among the first 31 reads: a read of 63 bases or more that is not one of the above gives way to one of its length that has such a list
    free = [i for i in range(31) if i not in special and len(reads[i]) >= 63]
    have = set()
    for i in range(31):
        if i not in free:
            have.update(event_counts(ptrs[i], [len(reads[i])]))
    for e in EDGES:
        if e in have:
            continue
        i, m = free[0], len(reads[free[0]])
        for tries in range(2000):
            r = make(tries % 4, m)
            p = oracle_pointers(o, r)
            if e in event_counts(p, [m]):
                reads[i], ptrs[i] = r, p
                have.update(event_counts(p, [m]))
                free.pop(0)
                break
    return reads, ptrs


@pytest.fixture(scope="module")
def gpu(medium_case):
    """the oracle, a context that takes the event lists and one made under MONI_MS_EVENTS=0"""
    from moni_align_amd import capi
    from oracle import orc
    idx = capi.Index(fi=medium_case.fi)
    ctx_ev = capi.Ctx(idx)
    old = os.environ.get("MONI_MS_EVENTS")
    os.environ["MONI_MS_EVENTS"] = "0"
    try:
        ctx_dense = capi.Ctx(idx)
    finally:
        if old is None:
            del os.environ["MONI_MS_EVENTS"]
        else:
            os.environ["MONI_MS_EVENTS"] = old
    yield orc.OracleIndex(medium_case.path), ctx_ev, ctx_dense
    ctx_ev.close()
    ctx_dense.close()
    idx.close()


@pytest.fixture(scope="module")
def mix(medium_case, gpu):
    return event_mix(medium_case, gpu[0])


def seed_both(gpu, reads, min_len=25, modes=(2, 0)):
    """the batch through both contexts and both filter modes against the oracle; returns the oracle's result"""
    o, ctx_ev, ctx_dense = gpu
    seq, offs = ragged(reads)
    want = o.seed_batch(seq, offs, min_len, True, 1000, threads=4)
    for mode in modes:
        got = []
        for ctx in (ctx_ev, ctx_dense):
            ctx.seed_prefilter(mode)
            try:
                ctx.upload(seq, offs)
                ctx.seed_run(min_len, True, 1000)
                g = ctx.seed_fetch()
                g["counters"] = ctx.counters()
            finally:
                ctx.seed_prefilter(1)
            assert_seeds_equal(g, want)
            got.append(g)
        assert got[0]["mems"].tobytes() == got[1]["mems"].tobytes() and np.array_equal(got[0]["occs"], got[1]["occs"]), mode
        assert np.array_equal(got[0]["read_mem_off"], got[1]["read_mem_off"]) and np.array_equal(got[0]["counters"], got[1]["counters"]), mode
        if mode == 0:
            assert np.array_equal(got[0]["counters"], want["counters"])
    return want


def test_the_mix_has_what_it_is_for(gpu, mix):
    reads, ptrs = mix
    assert {len(r) for r in reads} == set(LENS)
    assert all(len(reads[i]) != len(reads[i + 1]) for i in range(256))
    counts = [c for r, p in zip(reads[:31], ptrs[:31]) for c in event_counts(p, [len(r)])]
    for e in EDGES:
        assert e in counts, (e, sorted(set(counts)))
    every = [c for r, p in zip(reads, ptrs) for c in event_counts(p, [len(r)])]
    assert max(every) > 100 and sum(1 for c in every if c > 32) > 20          # the wrong strand: a jump at nearly every step
    assert (ptrs[39] >> np.uint64(40)).any() and reads[39][60] == ord("N") and reads[69][60] == 0xFF          # a wrapped decrement behind an N
    assert reads[19][0] == reads[29][149] == ord("N") and reads[49][0] >= 0x80 and reads[59][149] >= 0x80


@pytest.mark.parametrize("n", [257, 1, 31, 33])
def test_seeds_of_mixed_batches(gpu, mix, n):
    seed_both(gpu, mix[0][:n])


@pytest.mark.parametrize("top", [150, 161])
def test_seeds_by_mem_kernel_instance(gpu, mix, top):
    """no read beyond 160 bases: the five-word instances; up to 161: the eight-word ones, every read in the 2-bit comparison"""
    reads = [r for r in mix[0] if len(r) <= top]
    assert max(len(r) for r in reads) == top
    seed_both(gpu, reads)


def test_more_mems_than_slots(gpu, mix):
    """the chimeras hold five and six MEMs on one strand: counted without halves (report_mems), and seeded at a minimum length that gives many reads more"""
    _, ctx_ev, _ = gpu
    reads = mix[0][:33]
    ctx_ev.upload(*ragged(reads))
    ctx_ev.seed_run(25, True, 1000, report_mems=True)
    g = ctx_ev.seed_fetch()
    per = {}
    for m in g["mems"]:
        per[(int(m["read"]), int(m["mate"]))] = per.get((int(m["read"]), int(m["mate"])), 0) + 1
    assert per.get((3, 2), 0) > 4 and per.get((6, 0), 0) > 4 and per.get((9, 0), 0) > 4, per
    seed_both(gpu, mix[0][:64], min_len=12)


def test_short_batch_behind_a_long_one(gpu, mix):
    """the short batch's lists lie where the long batch's were, and an unfiltered dense walk behind a seeding run still gives every pointer"""
    o, ctx_ev, ctx_dense = gpu
    seed_both(gpu, mix[0], modes=(2,))
    part = mix[0][40:70]
    seed_both(gpu, part, modes=(2,))
    for ctx in (ctx_ev, ctx_dense):
        assert np.array_equal(ctx.ms_query_batch(*ragged(part)), np.concatenate(mix[1][40:70]))


def test_sam_text_under_both_settings(medium_case, gpu):
    _, ctx_ev, ctx_dense = gpu
    synth = medium_case.synth
    reads = synth.make_reads(medium_case.pg, 300, 150, seed=5)
    offs = np.arange(0, 301 * 150, 150, dtype=np.uint64)
    names, noff = synth.make_names(300)
    quals = np.full(reads.size, ord("I"), dtype=np.uint8)
    sam = [ctx.align_batch(reads.reshape(-1), offs, names, noff, quals, host_threads=4)[0] for ctx in (ctx_ev, ctx_dense)]
    assert sam[0] == sam[1] and sam[0].count(b"\n") >= 300
    rng = np.random.default_rng(7)
    pr = []
    for _ in range(150):
        sq = medium_case.pg.seqs[int(rng.integers(0, len(medium_case.pg.seqs)))]
        ins = int(max(210, rng.normal(350, 30)))
        at = int(rng.integers(0, len(sq) - ins))
        pr += [sq[at:at + 100].copy(), synth.revcomp(sq[None, at + ins - 100:at + ins])[0].copy()]
    poffs = np.arange(0, 301 * 100, 100, dtype=np.uint64)
    pnames = [("p%d/%d" % (i, k + 1)).encode() for i in range(150) for k in range(2)]
    pnoff = np.zeros(301, np.uint64)
    pnoff[1:] = np.cumsum([len(x) for x in pnames])
    pq = np.full(300 * 100, ord("I"), np.uint8)
    pe = []
    for ctx in (ctx_ev, ctx_dense):
        model = ctx.pe_learn(np.concatenate(pr), poffs)
        pe.append(ctx.pe_align(np.concatenate(pr), poffs, np.frombuffer(b"".join(pnames), np.uint8), pnoff, pq, model, host_threads=4)[0])
    assert pe[0] == pe[1] and pe[0].count(b"\n") >= 300
