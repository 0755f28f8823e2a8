"""The strand prefilter of the seeding stage (moni_seed_prefilter, csrc/prefilter_core.h) on the GPU: the seeds, the SAM text and the MS pointers are
what they are without it; the tasks it skips are the ones the rule names (a model of the rule in numpy below: no window of min_len bases with all
of its k-mers in the text), none of which has a MEM in the oracle's result; the work counters count the tasks that were walked; and it stands down
where it must.  On medium_case (360 k bases: k = 11)."""
import numpy as np
import pytest

from tests.parity import assert_seeds_equal

pytestmark = pytest.mark.gpu

MIN_LEN = 25
CODE = np.full(256, 4, dtype=np.int64)
for _b, _c in zip(b"ACTG", range(4)):
    CODE[_b] = _c
COMPL = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCATGCA"):
    COMPL[_a] = _b


def ragged(reads):
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    seq = np.concatenate(reads) if len(reads) and offs[-1] else np.zeros(0, np.uint8)
    return seq.astype(np.uint8), offs


def choose_k(n_text):
    e = 0
    while 4 ** e < n_text:
        e += 1
    return min(16, e + 1)


def kmers(codes, k):
    """value of the k-mer at every offset (base j in bits 2 j ..) and whether it holds only A / C / G / T"""
    nk = len(codes) - k + 1
    v = np.zeros(nk, dtype=np.int64)
    bad = np.zeros(nk, dtype=np.int64)
    for j in range(k):
        c = codes[j:j + nk]
        v |= (c & 3) << (2 * j)
        bad |= c >> 2
    return v, bad == 0


def text_table(text, k):
    v, ok = kmers(CODE[np.frombuffer(text, dtype=np.uint8)], k)
    return np.unique(v[ok])


def model_keep(pattern, min_len, k, table):
    """the rule of the issue for one strand-resolved pattern: True = the task is worked on"""
    codes = CODE[pattern]
    if (codes > 3).any() or min_len < k:
        return True
    if len(pattern) < min_len:
        return False
    v, _ = kmers(codes, k)
    at = np.searchsorted(table, v)
    present = (table[np.minimum(at, len(table) - 1)] == v).astype(np.int64)
    w = min_len - k + 1
    return bool(np.convolve(present, np.ones(w, dtype=np.int64), "valid").max() >= w)


def model_keeps(reads, min_len, k, table):
    out = np.zeros(2 * len(reads), dtype=bool)
    for i, r in enumerate(reads):
        out[2 * i] = model_keep(r, min_len, k, table)
        out[2 * i + 1] = model_keep(COMPL[r[::-1]], min_len, k, table)
    return out


@pytest.fixture(scope="module")
def gpu(medium_case):
    from moni_align_amd import capi
    from oracle import orc
    idx = capi.Index(fi=medium_case.fi)
    ctx = capi.Ctx(idx)
    yield orc.OracleIndex(medium_case.path), ctx
    ctx.close()
    idx.close()


def ragged_reads(mc):
    rng = np.random.default_rng(5)          # the set of test_gpu_seed.py::test_seeds_ragged_edge_cases
    base = mc.synth.make_reads(mc.pg, 3000, 250, seed=9, sub_rate=0.03, indel_rate=0.003)
    reads = [r[: int(rng.integers(1, 251))].copy() for r in base]
    reads.append(np.zeros(0, np.uint8))
    reads.append(np.frombuffer(b"N" * 60, dtype=np.uint8))
    reads.append(np.frombuffer(b"acgtacgtacgtacgtacgtacgtacgtacgtacgt", dtype=np.uint8))
    x = base[0].copy(); x[40:45] = ord("N"); reads.append(x)
    reads.append(np.frombuffer(bytes(mc.fi.text[100:400]), dtype=np.uint8))
    return reads


@pytest.fixture(scope="module")
def runs(medium_case, gpu):
    """both read sets, each through the oracle once and through the GPU in mode 2 and mode 0"""
    o, ctx = gpu
    k = choose_k(len(medium_case.text))
    assert k == 11
    table = text_table(medium_case.text, k)
    out = {}
    for name, reads in (("150bp", list(medium_case.synth.make_reads(medium_case.pg, 5000, 150, seed=77))), ("ragged", ragged_reads(medium_case))):
        seq, offs = ragged(reads)
        d = {"reads": reads, "want": o.seed_batch(seq, offs, MIN_LEN, True, 1000, threads=4), "keep": model_keeps(reads, MIN_LEN, k, table), "table": table, "k": k}
        for mode in (2, 0):
            ctx.seed_prefilter(mode)
            ctx.upload(seq, offs)
            ctx.seed_run(MIN_LEN, True, 1000)
            d[mode] = {"got": ctx.seed_fetch(), "counters": ctx.counters(), "stats": ctx.seed_prefilter_stats()}
        ctx.seed_prefilter(1)
        out[name] = d
    return out


@pytest.mark.parametrize("name", ["150bp", "ragged"])
@pytest.mark.parametrize("mode", [2, 0])
def test_seeds_against_the_oracle(runs, name, mode):
    d = runs[name]
    assert_seeds_equal(d[mode]["got"], d["want"])
    if mode == 0:
        assert np.array_equal(d[0]["counters"], d["want"]["counters"])
        assert d[0]["stats"]["skipped"] == 0 and d[0]["stats"]["lookups"] == 0


@pytest.mark.parametrize("name", ["150bp", "ragged"])
def test_filter_statistics(runs, name):
    d = runs[name]
    reads, want, keep, st = d["reads"], d["want"], d["keep"], d[2]["stats"]
    n_tasks = 2 * len(reads)
    lens = np.repeat(np.array([len(r) for r in reads], dtype=np.int64), 2)
    has_mem = np.zeros(n_tasks, dtype=bool)          # the oracle's MEMs (and halves) per task: strand 1 carries mate 2
    has_mem[2 * want["read"].astype(np.int64) + (want["mate"].astype(np.int64) >> 1)] = True
    print("%s: %d tasks, %d skipped (the rule: %d), %d without a MEM in the oracle's result, %d lookups, density %.4f; S J C with the filter %s, without %s"
          % (name, st["tasks"], st["skipped"], int((~keep).sum()), int((~has_mem).sum()), st["lookups"], st["density"], d[2]["counters"][[0, 1, 3]], d[0]["counters"][[0, 1, 3]]))
    assert st["tasks"] == n_tasks
    assert st["skipped"] > 0
    assert abs(st["density"] - len(d["table"]) / 4.0 ** d["k"]) < 2e-6
    assert st["skipped"] == int((~keep).sum())          # the tasks the rule names, no others
    assert not (has_mem & ~keep).any()                   # every skipped task has no MEM in the oracle's result
    assert 2 * st["skipped"] >= int((~has_mem).sum())    # of the oracle's no-MEM tasks at least half are skipped
    assert int(d[2]["counters"][0]) == int(lens[keep].sum())          # steps walked: the live tasks' lengths
    assert d[2]["counters"][1] <= d[0]["counters"][1] and d[2]["counters"][3] <= d[0]["counters"][3]
    assert d[2]["counters"][2] == d[0]["counters"][2]    # the same seeds, the same phi walks


def test_stands_down_for_a_short_min_len(runs, gpu):
    o, ctx = gpu
    seq, offs = ragged(runs["ragged"]["reads"])
    ctx.seed_prefilter(2)
    ctx.upload(seq, offs)
    ctx.seed_run(12, True, 1000)          # a window of 12 bases holds two 11-mers: the filter still works
    assert ctx.seed_prefilter_stats()["skipped"] > 0
    ctx.seed_run(10, True, 1000)          # min_len below k = 11
    st = ctx.seed_prefilter_stats()
    ctx.seed_prefilter(1)
    assert st["tasks"] == 2 * (len(offs) - 1) and st["skipped"] == 0 and st["lookups"] == 0


def test_min_len_12_below_k_skips_nothing(medium_case, runs, monkeypatch):
    """min_len = 12 on the ragged set.  medium_case's own table has k = 11, for which a window of 12 bases still holds two k-mers and the filter
    works (the test above: reads shorter than 12 bases alone are skipped outright); the case "min_len below k" is made on the same index with
    13-mers for a table (MONI_PREFILTER_K): nothing is skipped, no lookup is made."""
    from moni_align_amd import capi
    monkeypatch.setenv("MONI_PREFILTER_K", "13")
    idx = capi.Index(fi=medium_case.fi)
    ctx = capi.Ctx(idx)
    try:
        seq, offs = ragged(runs["ragged"]["reads"])
        ctx.seed_prefilter(2)
        ctx.upload(seq, offs)
        ctx.seed_run(12, True, 1000)
        st = ctx.seed_prefilter_stats()
        assert st["tasks"] == 2 * (len(offs) - 1) and st["skipped"] == 0 and st["lookups"] == 0
        ctx.seed_run(MIN_LEN, True, 1000)          # (the same table filters at min_len = 25)
        assert ctx.seed_prefilter_stats()["skipped"] > 0
        assert_seeds_equal(ctx.seed_fetch(), runs["ragged"]["want"])
    finally:
        ctx.close()
        idx.close()


def test_stands_down_for_a_dense_table(tmp_path, monkeypatch):
    """a random 3 kb text with 5-mers for a table (k from the formula keeps a random text under a quarter: the tuning variable makes the dense case):
    density over 0.25, nothing skipped, the seeds the oracle's"""
    from moni_align_amd import capi, index_build, synth
    from oracle import orc
    pg = synth.make_pangenome(3000, 1, site_spacing=500)
    fi = index_build.build_from_pangenome(pg, device="cpu")
    path = str(tmp_path / "dense.mfi")
    fi.save(path)
    monkeypatch.setenv("MONI_PREFILTER_K", "5")
    idx = capi.Index(fi=fi)
    ctx = capi.Ctx(idx)
    try:
        reads = list(synth.make_reads(pg, 500, 100, seed=4))
        seq, offs = ragged(reads)
        ctx.seed_prefilter(2)
        ctx.upload(seq, offs)
        ctx.seed_run(MIN_LEN, True, 1000)
        st = ctx.seed_prefilter_stats()
        print("dense table:", st)
        assert st["density"] > 0.25
        assert st["tasks"] == 1000 and st["skipped"] == 0 and st["lookups"] == 0
        assert_seeds_equal(ctx.seed_fetch(), orc.OracleIndex(path).seed_batch(seq, offs, MIN_LEN, True, 1000, threads=4))
    finally:
        ctx.close()
        idx.close()


def test_sam_identical_single_end(medium_case, gpu):
    o, ctx = gpu
    reads = medium_case.synth.make_reads(medium_case.pg, 3000, 150, seed=88)
    seq, offs = ragged(list(reads))
    names, noff = medium_case.synth.make_names(len(reads))
    quals = np.full(seq.size, ord("I"), dtype=np.uint8)
    sam = {}
    for mode in (1, 0):
        ctx.seed_prefilter(mode)
        sam[mode], _ = ctx.align_batch(seq, offs, names, noff, quals, host_threads=4)
        st = ctx.seed_prefilter_stats()
        assert (st["skipped"] > 0) == (mode == 1), st          # mode 1 filters in the align path
    ctx.seed_prefilter(1)
    ctx.upload(seq, offs)
    ctx.seed_run(MIN_LEN, True, 1000)                          # ... and not in seed_run
    assert ctx.seed_prefilter_stats()["skipped"] == 0
    assert sam[1] == sam[0]


def test_sam_identical_paired(medium_case, gpu):
    o, ctx = gpu
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
    ctx.seed_prefilter(0)
    model = ctx.pe_learn(seq, offs)
    sam = {}
    for mode in (1, 0):
        ctx.seed_prefilter(mode)
        sam[mode], _ = ctx.pe_align(seq, offs, names, noff, quals, model, host_threads=4)
        st = ctx.seed_prefilter_stats()
        assert (st["skipped"] > 0) == (mode == 1), st
    ctx.seed_prefilter(1)
    assert sam[1] == sam[0]


def test_ms_pointers_unchanged_after_a_filtered_run(medium_case, gpu):
    o, ctx = gpu
    reads = medium_case.synth.make_reads(medium_case.pg, 500, 150, seed=150)
    seq, offs = ragged(list(reads))
    before = ctx.ms_query_batch(seq, offs)
    ctx.seed_prefilter(2)
    ctx.upload(seq, offs)
    ctx.seed_run(MIN_LEN, True, 1000)
    assert ctx.seed_prefilter_stats()["skipped"] > 0
    after = ctx.ms_query_batch(seq, offs)
    ctx.seed_prefilter(1)
    assert np.array_equal(before, after)
    for i in (0, 250, 499):          # ... and they are the oracle's
        assert np.array_equal(after[300 * i:300 * i + 150], o.ms_query(reads[i].tobytes())), i
