"""chain_runs_kernel chains the runs of anchors of most reads with one lane per run, four reads per wavefront: the small plain instance of
chain_plan_kernel stops behind the runs for a read of at most 16 runs of at most AF_RUN_LEN anchors, leaves its sorted anchors in HBM, and the new kernel
does the DP, the chain ends and starts, the backtracking, the keep test, the order of the chains (one insertion sort up to 16, the introsort beyond), the
lifts and the chain table.  The bytes must not show any of that: the SAM text of
moni_align_run equals the oracle's, equals the run with MONI_AF_RUNS=0 (every read chained in place) and the run with MONI_AF_DBG=64 (the general instances,
serial sorts), on batches built for the places where the route takes another path.  Every batch asserts, from the seeds the GPU fetches (a model of the
chaining over them) and from the counter of the reads that took the route, that it holds the case it is there for."""
import numpy as np
import pytest

from tests.chain_runs_model import CHAINS, L0_SEEDS, NODES, RUN_LEN, SLOTS, models
from tests.test_gpu_chain_diet import GAP, fetch_seeds, repeat_batch
from tests.test_gpu_prep_tail import _arrays, _sub
from tests.test_gpu_render import ACGT, Case, oracle_text, run, same

pytestmark = pytest.mark.gpu


def three_runs(ctx, arr, want, monkeypatch):
    """the route, MONI_AF_RUNS=0 and MONI_AF_DBG=64 against the oracle's text; returns the number of reads that took the route"""
    got, st = run(ctx, arr)
    same(got, want)
    with monkeypatch.context() as mp:
        mp.setenv("MONI_AF_RUNS", "0")
        got_off, st_off = run(ctx, arr)
    same(got_off, want)
    assert st_off["runs_routed"] == 0
    with monkeypatch.context() as mp:
        mp.setenv("MONI_AF_DBG", "64")
        got_serial, st_serial = run(ctx, arr)
    same(got_serial, want)
    assert st_serial["runs_routed"] == 0
    return st["runs_routed"]


def short_seed_reads(seq, rng, n):
    """reads with one seed of 36 bases (the text's) between random bases: no chain scores above min_chain_score = 40, the read has no chain start"""
    out = []
    for _ in range(n):
        p = int(rng.integers(0, len(seq) - 36))
        out.append(np.concatenate([ACGT[rng.integers(0, 4, size=40)], seq[p:p + 36], ACGT[rng.integers(0, 4, size=44)]]))
    return out


@pytest.fixture(scope="module")
def repeats(tmp_path_factory):
    """test_gpu_chain_diet's families of segment copies (4 .. 24 copies: as many runs; the copies of a family mostly equal: equal chain scores), its
    120 + 30 + 30 reads, and reads without a chain start; 3 reads short of a multiple of 4, the families shuffled so that neighbours differ"""
    seq, reads = repeat_batch()
    rng = np.random.default_rng(17)
    reads += short_seed_reads(seq, rng, 9)
    reads = [reads[k] for k in rng.permutation(len(reads))]
    while len(reads) % 4 != 1:
        reads.pop()
    c = Case(tmp_path_factory.mktemp("chain_runs"), [seq], ["rep"])
    arr = _arrays(reads)
    yield c, arr, oracle_text(c.oracle, arr)
    c.close()


def test_runs_at_the_slots_and_both_routes_in_one_wavefront(repeats, monkeypatch):
    c, arr, want = repeats
    ms = models(fetch_seeds(c.ctx, arr))
    n_reads = len(ms)
    assert n_reads % 4 != 0
    runs = [m["n_runs"] for m in ms]
    assert any(m["n_runs"] == SLOTS and m["routed"] for m in ms) and any(m["n_runs"] == SLOTS + 1 and not m["gate"] and m["n"] <= NODES for m in ms), sorted(set(runs))
    assert any(m["steps"] >= 2 and m["routed"] for m in ms), "no routed read whose F < MSC walk takes more than one step"
    assert any(m["n"] > 0 and m["starts"] == 0 and m["gate"] for m in ms), "no routed read without a chain start"
    assert any(m["equal_scores"] and m["routed"] and m["kept"] >= 4 for m in ms), "no routed read whose chains all score the same"
    assert any(m["multi_start_dropped"] and m["routed"] for m in ms), "no routed read with a run of several chain starts, one of them dropped"
    assert any(m["tied"] and m["routed"] for m in ms)
    assert any(m["routed"] and m["kept"] <= 16 for m in ms) and sum(1 for m in ms if m["routed"] and m["kept"] > 16) >= 20      # one insertion sort; the introsort
    # Four consecutive entries of the small instance's list share a wavefront of the new kernel.  classify_kernel appends to that list wave by wave (64
    # reads, in read order inside a wave; the waves in the order of their atomics), so which four meet is not known here.  What is: the reads of the list
    # in read order change their route 150 times and more, and a run of one route is never 64 long - so whatever the waves' order, wavefronts that hold
    # both routes are certain, though this test cannot name them.
    l0 = [m for m in ms if m["n"] <= NODES and m["seeds"] <= L0_SEEDS]
    assert len(l0) >= n_reads - 60
    flips = [k for k in range(1, len(l0)) if l0[k]["routed"] != l0[k - 1]["routed"]]
    assert len(flips) >= 150 and max(b - a for a, b in zip([0] + flips, flips + [len(l0)])) < 32, len(flips)
    routed = three_runs(c.ctx, arr, want, monkeypatch)
    expect = sum(1 for m in ms if m["routed"])
    assert not any(m["gate"] and m["starts"] >= CHAINS - 4 for m in ms)          # (no read near the cap, where the model's order of tied anchors could decide)
    assert 0 < expect < n_reads and routed == expect, (routed, expect)


def long_run_batch(seed=9):
    """two copies of a unique stretch; reads of up to 200 bases (longer reads go through the middle instance, which has no such route) made of pieces of 50
    matching bases (a seed and its two halves: three anchors) and of 25 (one anchor), a substituted base between them: runs of 3 .. 10 anchors"""
    from moni_align_amd import synth
    rng = np.random.default_rng(seed)
    uniq = ACGT[rng.integers(0, 4, size=6000)]
    seq = np.concatenate([uniq, ACGT[rng.integers(0, 4, size=GAP + 400)], uniq])
    shapes = [(a, b) for a in (1, 2, 3) for b in (0, 1, 2, 3) if 51 * a + 26 * b - 1 <= 200]
    reads = []
    for k in range(80):
        a, b = shapes[k % len(shapes)]
        lens = [50] * a + [25] * b
        lens = [lens[q] for q in rng.permutation(len(lens))]
        p = int(rng.integers(0, len(uniq) - 220))
        cuts = np.cumsum([x + 1 for x in lens])[:-1] - 1
        r = _sub(uniq[p:p + sum(lens) + len(lens) - 1], [int(x) for x in cuts])
        reads.append(r if k % 2 else synth.revcomp(r[None, :])[0].copy())
    return seq, reads


def test_the_longest_run_at_the_cap_and_one_above(tmp_path, monkeypatch):
    seq, reads = long_run_batch()
    c = Case(tmp_path, [seq], ["uniq"])
    try:
        arr = _arrays(reads)
        ms = models(fetch_seeds(c.ctx, arr))
        lens = sorted(set(m["max_run"] for m in ms))
        assert any(m["max_run"] == RUN_LEN and m["routed"] for m in ms) and any(m["max_run"] == RUN_LEN + 1 and not m["gate"] and m["n"] <= NODES for m in ms), lens
        assert all(m["starts"] <= 16 for m in ms) and max(len(r) for r in reads) <= 200
        routed = three_runs(c.ctx, arr, oracle_text(c.oracle, arr), monkeypatch)
        assert routed == sum(1 for m in ms if m["routed"]) and 0 < routed < len(ms)
    finally:
        c.close()


def kept_chain_batch(seed=21):
    """families of 16 copies of A + B (45 bases each: seeds shorter than 2 x min_len have no halves), the copies 600 random bases apart: a read A + one other
    base + B has two seeds with 16 occurrences each, 16 runs, one chain per run: 16 kept chains, all of one score, in the order of the sorted starts.  In the
    second family one copy holds B + A: its run has two chain starts and keeps both, 17 kept chains in 16 runs, which go through the introsort."""
    rng = np.random.default_rng(seed)
    parts, fam_reads = [], []
    for swapped in (0, 1):
        a, b = ACGT[rng.integers(0, 4, size=45)], ACGT[rng.integers(0, 4, size=45)]
        for k in range(16):
            mid = ACGT[[0]]          # (the reads hold a C there: no match runs on from A into B)
            body = np.concatenate([b, mid, a]) if (swapped and k == 7) else np.concatenate([a, mid, b])
            parts.append(np.concatenate([ACGT[rng.integers(0, 4, size=600)], body]))
        fam_reads.append(np.concatenate([a, ACGT[[1]], b]))
    seq = np.concatenate(parts + [ACGT[rng.integers(0, 4, size=600)]])
    from moni_align_amd import synth
    reads = []
    for k in range(20):
        r = fam_reads[k % 2]
        reads.append(r if k % 4 < 2 else synth.revcomp(r[None, :])[0].copy())
    return seq, reads


def test_sixteen_and_seventeen_kept_chains(tmp_path, monkeypatch):
    seq, reads = kept_chain_batch()
    c = Case(tmp_path, [seq], ["fam"])
    try:
        arr = _arrays(reads)
        ms = models(fetch_seeds(c.ctx, arr))
        kept = sorted(set((m["n_runs"], m["kept"]) for m in ms))
        assert all(m["gate"] and not m["tied"] for m in ms), kept
        assert sum(1 for m in ms if m["kept"] == 16) == 10 and sum(1 for m in ms if m["kept"] == 17 and m["n_runs"] == SLOTS) == 10, kept
        routed = three_runs(c.ctx, arr, oracle_text(c.oracle, arr), monkeypatch)
        assert routed == 20
    finally:
        c.close()


def start_cap_batch(seed=33):
    """reads at the cap of chain starts, where the new kernel hands a read to the large instance's list (LEVEL 1 runs behind it).  Pieces of 45 bases
    (no halves), an A on both sides of each in the text and a C between them in the read (no match runs on).  Family 0: 16 copies of C' B' A' in the
    text, the read is A' B' C': three anchors per run in falling read order, none chains to another, three chain starts per run: 16 runs, 48 starts,
    48 kept chains.  Family 1: the same with four pieces in one of the copies (D C B A; the read is A B C D): 15 x 3 + 4 = 49 starts in 16 runs."""
    from moni_align_amd import synth
    rng = np.random.default_rng(seed)
    A1 = ACGT[[0]]
    parts, fam_reads = [], []
    for fam in (0, 1):
        pcs = [ACGT[rng.integers(0, 4, size=45)] for _ in range(3 + fam)]
        for k in range(16):
            use = pcs if (fam and k == 5) else pcs[:3]
            body = np.concatenate([A1] + [x for q in reversed(use) for x in (q, A1)])
            parts.append(np.concatenate([ACGT[rng.integers(0, 4, size=600)], body]))
        fam_reads.append(np.concatenate([x for q in pcs for x in (q, ACGT[[1]])][:-1]))
    seq = np.concatenate(parts + [ACGT[rng.integers(0, 4, size=600)]])
    reads = []
    for k in range(22):
        r = fam_reads[(k // 3) % 2]          # (neighbours in the list: both kinds meet in wavefronts of the new kernel)
        reads.append(r if k % 4 < 2 else synth.revcomp(r[None, :])[0].copy())
    return seq, reads


def test_the_cap_of_chain_starts_and_the_hand_over_to_the_large_instance(tmp_path, monkeypatch):
    seq, reads = start_cap_batch()
    c = Case(tmp_path, [seq], ["cap"])
    try:
        arr = _arrays(reads)
        ms = models(fetch_seeds(c.ctx, arr))
        seen = sorted(set((m["n_runs"], m["max_run"], m["starts"], m["kept"]) for m in ms))
        assert all(m["gate"] and not m["tied"] and m["n_runs"] == SLOTS for m in ms) and max(len(r) for r in reads) <= 200, seen
        at_cap = sum(1 for m in ms if m["starts"] == CHAINS and m["kept"] == CHAINS and m["routed"])
        above = sum(1 for m in ms if m["starts"] == CHAINS + 1 and not m["routed"])
        assert at_cap >= 8 and above >= 8 and at_cap + above == len(ms), seen
        routed = three_runs(c.ctx, arr, oracle_text(c.oracle, arr), monkeypatch)
        assert routed == at_cap          # the reads of 49 starts pass the test behind the runs and leave the new kernel for the large instance
    finally:
        c.close()


def test_an_earlier_batch_leaves_nothing_behind(repeats, tmp_path, monkeypatch):
    """the same batch twice on one context with another batch between them, and the other batch after it: reads change their route from launch to launch"""
    c, arr, want = repeats
    rng = np.random.default_rng(3)
    seq = c.pg.seqs[0]
    other = short_seed_reads(seq, rng, 30)
    for k in range(len(arr[1]) - 1 - 30):          # reads of the unique stretch at the text's end: one run, routed, where the first batch's neighbours were not
        p = int(rng.integers(len(seq) - 2000, len(seq) - 130))
        other.append(_sub(seq[p:p + 120], [60]))
    arr2 = _arrays(other)
    want2 = oracle_text(c.oracle, arr2)
    got, st1 = run(c.ctx, arr)
    same(got, want)
    got2, st2 = run(c.ctx, arr2)
    same(got2, want2)
    got3, st3 = run(c.ctx, arr)
    same(got3, want)
    assert st1["runs_routed"] == st3["runs_routed"] > 0 and st2["runs_routed"] >= len(other) - 30 > st1["runs_routed"]
