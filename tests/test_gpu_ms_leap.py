"""The leaping walk of the seeding stage on the GPU (ms_lf_leap_kernel; seed_core.h: ms_task_events_leap), no tolerance anywhere.  The sampled inverse
suffix array that the index builds on the device is compared entry by entry with a suffix array made here; about 2000 reads - simulated reads, the
edge reads of tests/test_host_ms_leap.py and the batches of tests/test_host_ms_events.py - are seeded by a context that leaps and by one made under
MONI_MS_LEAP=0, with the strand prefilter on and off, and compared with each other byte for byte (seeds, occurrences, the counters S and J) and with the
oracle; the leaping context must have leapt.  One single-end batch as SAM text against the oracle, one paired batch between the two settings."""
import os

import numpy as np
import pytest

from tests.parity import assert_seeds_equal
from tests.test_host_ms_events import edge_mix
from tests.test_host_ms_leap import leap_mix
from tests.test_host_ms_stage import length_mix, ragged

pytestmark = pytest.mark.gpu
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def suffix_array(s):
    """prefix doubling; s ends with its unique smallest byte"""
    n, k = len(s), 1
    rk = s.astype(np.int64)
    while True:
        rk2 = np.zeros(n, np.int64)
        if k < n:
            rk2[:n - k] = rk[k:] + 1
        order = np.lexsort((rk2, rk))
        a, b = rk[order], rk2[order]
        new = np.empty(n, np.int64)
        new[order] = np.cumsum(np.concatenate([[0], ((a[1:] != a[:-1]) | (b[1:] != b[:-1])).astype(np.int64)]))
        rk = new
        if int(rk.max()) == n - 1:
            return order
        k *= 2


def ctx_without_leap(capi, idx):
    old = os.environ.get("MONI_MS_LEAP")
    os.environ["MONI_MS_LEAP"] = "0"
    try:
        return capi.Ctx(idx)
    finally:
        if old is None:
            del os.environ["MONI_MS_LEAP"]
        else:
            os.environ["MONI_MS_LEAP"] = old


@pytest.fixture(scope="module")
def gpu(medium_case):
    from moni_align_amd import capi
    from oracle import orc
    idx = capi.Index(fi=medium_case.fi)
    ctx_leap, ctx_step = capi.Ctx(idx), ctx_without_leap(capi, idx)
    yield orc.OracleIndex(medium_case.path), idx, ctx_leap, ctx_step
    ctx_leap.close()
    ctx_step.close()
    idx.close()


@pytest.fixture(scope="module")
def batch(medium_case):
    """about 2000 reads, neighbouring lanes of different kinds"""
    sim = medium_case.synth.make_reads(medium_case.pg, 1500, 150, seed=21, sub_rate=0.02)
    reads = [sim[i].copy() for i in range(len(sim))] + leap_mix(medium_case, 6, 120)[0] + length_mix(medium_case, 60, 4) + edge_mix(medium_case, 5)
    order = np.random.default_rng(3).permutation(len(reads))
    return [reads[k] for k in order]


def check_table(case, idx):
    fi = case.fi
    n = int(fi.n)
    text = np.frombuffer(bytes(fi.text), dtype=np.uint8)[:n - 1]
    sa = suffix_array(np.concatenate([text, np.zeros(1, np.uint8)]))
    isa = np.empty(n, np.int64)
    isa[sa] = np.arange(n)
    tab = idx.leap_table()
    s = tab["stride"]
    assert s == 16 and len(tab["isa"]) == (n - 1) // s + 1
    starts = np.asarray(fi.starts, dtype=np.int64)
    run, off = (tab["isa"] & np.uint64(0xFFFFFFFF)).astype(np.int64), (tab["isa"] >> np.uint64(32)).astype(np.int64)
    assert (run < int(fi.r)).all() and (starts[run] + off < starts[run + 1]).all()
    assert np.array_equal(starts[run] + off, isa[::s])
    ok = np.concatenate([np.isin(text, ACGT), np.zeros(256, bool)]).astype(np.int64)          # clean: the run of A / C / G / T bytes from t on, at most 255
    z = np.concatenate([[0], np.cumsum(1 - ok)])
    t = np.arange(0, n, s)
    first_bad = np.searchsorted(z, z[t], side="right") - 1          # the first position >= t that is not A / C / G / T
    assert np.array_equal(tab["clean"], np.minimum(first_bad - t, 255).astype(np.uint8))


def test_table_small(small_case):
    from moni_align_amd import capi
    idx = capi.Index(fi=small_case.fi)
    try:
        check_table(small_case, idx)
    finally:
        idx.close()


def test_table_medium(medium_case, gpu):
    check_table(medium_case, gpu[1])


def test_no_table_under_the_switch(small_case):
    from moni_align_amd import capi
    old = os.environ.get("MONI_MS_LEAP")
    os.environ["MONI_MS_LEAP"] = "0"
    try:
        idx = capi.Index(fi=small_case.fi)
    finally:
        if old is None:
            del os.environ["MONI_MS_LEAP"]
        else:
            os.environ["MONI_MS_LEAP"] = old
    try:
        assert idx.leap_table()["stride"] == 0
        with_table = capi.Index(fi=small_case.fi)
        assert with_table.device_bytes > idx.device_bytes
        with_table.close()
    finally:
        idx.close()


@pytest.mark.parametrize("mode", [2, 0], ids=["filtered", "every-task"])
def test_seeds_with_and_without_leaps(gpu, batch, mode):
    o, _, ctx_leap, ctx_step = gpu
    seq, offs = ragged(batch)
    want = o.seed_batch(seq, offs, 25, True, 1000, threads=4)
    got = []
    for ctx in (ctx_leap, ctx_step):
        ctx.seed_prefilter(mode)
        try:
            ctx.upload(seq, offs)
            ctx.seed_run(25, True, 1000)
            g = ctx.seed_fetch()
            g["counters"] = ctx.counters()
            g["leap"] = ctx.ms_leap_stats()
        finally:
            ctx.seed_prefilter(1)
        assert_seeds_equal(g, want)
        got.append(g)
    assert got[0]["mems"].tobytes() == got[1]["mems"].tobytes() and np.array_equal(got[0]["occs"], got[1]["occs"])
    assert np.array_equal(got[0]["read_mem_off"], got[1]["read_mem_off"])
    assert np.array_equal(got[0]["counters"], got[1]["counters"])          # S and J: the reference walk's steps and jumps
    if mode == 0:
        assert np.array_equal(got[0]["counters"], want["counters"])
    lp, st = got[0]["leap"], got[1]["leap"]
    print(lp, got[0]["counters"])
    assert lp["stride"] == 16 and lp["leaps"] > 0 and lp["steps_leapt"] >= 9 * lp["leaps"] and lp["comparisons"] >= lp["leaps"]          # (a leap crosses more than K_MIN = 8 steps)
    assert st["leaps"] == 0 and st["steps_leapt"] == 0 and st["comparisons"] == 0


def test_sam_text(medium_case, gpu):
    from oracle import orc
    o, _, ctx_leap, ctx_step = gpu
    synth = medium_case.synth
    reads = synth.make_reads(medium_case.pg, 300, 150, seed=5)
    offs = np.arange(0, 301 * 150, 150, dtype=np.uint64)
    names, noff = synth.make_names(300)
    quals = np.full(reads.size, ord("I"), dtype=np.uint8)
    want, _ = orc.align_batch(o, reads.reshape(-1), offs, names, noff, quals, threads=4)
    sam = ctx_leap.align_batch(reads.reshape(-1), offs, names, noff, quals, host_threads=4)[0]
    assert sam == want and ctx_leap.ms_leap_stats()["leaps"] > 0
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
    for ctx in (ctx_leap, ctx_step):
        model = ctx.pe_learn(np.concatenate(pr), poffs)
        pe.append(ctx.pe_align(np.concatenate(pr), poffs, np.frombuffer(b"".join(pnames), np.uint8), pnoff, pq, model, host_threads=4)[0])
    assert pe[0] == pe[1] and pe[0].count(b"\n") >= 300
