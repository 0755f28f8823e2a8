"""chain_plan_kernel runs the chaining DP in 32-bit integers (chain_core.h), keeps the values that are the same in every lane in scalar registers, asks for
all anchors of a read at once, and leaves the serial sorts and the 64-bit DP to the general instances that MONI_AF_DBG=64 (or chaining parameters beyond
cc_narrow_ok) launches.  The bytes must not show any of that: the SAM text of
moni_align_run equals the oracle's and equals the run with MONI_AF_DBG=64, on batches built for the places where the code takes another path - reads of
exactly 16 and 17 anchors (one insertion sort / the introsort loop), 64 and 65 (one pass of the lanes / two), 96 and more than 96 (the small instance's
capacity / the next instance), tied sort keys, runs with several chain starts, chains that leave the F < MSC walk after more than one step - and under
chaining parameters that run the wide form or the early exits of the predecessor loop.  Every test asserts on its own batch, from the seeds the GPU
fetches, that the batch holds the case it is there for."""
import numpy as np
import pytest

from tests.test_gpu_prep_tail import _arrays, _sub
from tests.test_gpu_render import ACGT, Case, oracle_text, run, same

pytestmark = pytest.mark.gpu

COPIES = (4, 5, 6, 8, 11, 12, 13, 16, 17, 20, 24)      # anchors of a read = seeds x copies: 16 = 2 x 8 = 4 x 4, 17 = 6 + 6 + 5, 64 = 4 x 16, 65 = 5 x 13, 96 = 4 x 24 = 6 x 16 ...
SEG, GAP, READ = 300, 250, 120
NARROW_MAX_DIST = 1 << 28                                # CC_NARROW_MAX_DIST (chain_core.h)
DEFAULTS = dict(min_len=25, freq_thr=0.5, max_dist_x=500, max_dist_y=100, max_iter=10, max_pred=5, min_chain_score=40)      # moni_align_params_default


def repeat_batch(seed=3, per_family=60):
    """one sequence: SEG-base segments in COPIES copies each (two substituted bases per copy, so the copies that share a seed vary), random bases between
    the copies; per_family reads of READ bases per segment with 0 .. 6 substituted bases, both strands"""
    from moni_align_amd import synth
    rng = np.random.default_rng(seed)
    parts, fams = [], []
    for n_copy in COPIES:
        seg = ACGT[rng.integers(0, 4, size=SEG)]
        mine = [seg if k < n_copy - 2 else _sub(seg, [int(x) for x in rng.choice(SEG, size=2, replace=False)]) for k in range(n_copy)]
        fams.append(mine)
        parts += [np.concatenate([x, ACGT[rng.integers(0, 4, size=GAP)]]) for x in mine]
    # a unique stretch, and reads that skip 150 of its bases twice: 120 + 30 + 30 bases whose three seeds chain at a loss (beta > alpha), so the chain's
    # end scores less than its first anchor and the F < MSC walk goes back two steps
    rng_u = np.random.default_rng(seed + 1000)
    uniq = ACGT[rng_u.integers(0, 4, size=2000)]
    seq = np.concatenate([parts[k] for k in rng.permutation(len(parts))] + [uniq])
    reads = []
    for _ in range(12):
        p = int(rng_u.integers(0, len(uniq) - 480))
        r = np.concatenate([uniq[p:p + 120], uniq[p + 270:p + 300], uniq[p + 450:p + 480]])
        reads.append(r if rng_u.random() < 0.5 else synth.revcomp(r[None, :])[0].copy())
    for mine in fams:
        for k in range(per_family):
            x = mine[int(rng.integers(0, len(mine)))]
            p = int(rng.integers(0, SEG - READ))
            r = _sub(x[p:p + READ], [int(v) for v in rng.choice(READ, size=k % 7, replace=False)])
            reads.append(r if rng.random() < 0.5 else synth.revcomp(r[None, :])[0].copy())
    return seq, reads


def anchors_of(seeds, prm=DEFAULTS):
    """per read: (x, rpos, len, mate) of its anchors after seed_freq_filter, in populate_anchors' order"""
    mems, occs, rmo = seeds["mems"], seeds["occs"], seeds["read_mem_off"]
    out = []
    for r in range(len(rmo) - 1):
        ms = mems[int(rmo[r]):int(rmo[r + 1])]
        total = int(ms["occ_cnt"].sum())
        an = []
        for m in ms:
            if total and int(m["occ_cnt"]) / total > prm["freq_thr"]:
                continue
            for o in occs[int(m["occ_off"]):int(m["occ_off"]) + int(m["occ_cnt"])]:
                an.append((int(o) + int(m["len"]) - 1, int(m["rpos"]), int(m["len"]), int(m["mate"])))
        out.append(an)
    return out


def chain_model(an, prm=DEFAULTS):
    """the chaining DP of chain.hpp:278-400 over one read's anchors (single-end: no pair of different mates chains), sorted by x with a stable sort: the
    order of tied anchors may differ from libstdc++'s, which moves no anchor between runs.  Returns (has tied keys, most chain starts in one run, most steps
    of a chain end's F < MSC walk)."""
    import math
    an = sorted(an, key=lambda a: a[0])
    n = len(an)
    tied = any(an[i][0] == an[i - 1][0] for i in range(1, n))
    f, p, t, msc = [0] * n, [0] * n, [0] * n, [0] * n
    avg = np.float32(sum(a[2] for a in an)) / np.float32(n) if n else 0.0
    lb = 0
    for i in range(n):
        x_i, y_i, w_i, mate_i = an[i]
        max_f, max_j, n_pred = w_i, -1, 0
        if i - lb > prm["max_iter"]:
            lb = i - prm["max_iter"]
        j = i - 1
        while j >= lb:
            x_j, y_j, _, mate_j = an[j]
            jj = j
            j -= 1
            if mate_i != mate_j:
                continue
            if x_i > x_j + prm["max_dist_x"]:
                lb = jj
                continue
            x_d, y_d = x_i - x_j, y_i - y_j
            l = abs(y_d - x_d)
            if y_j >= y_i or y_d > prm["max_dist_y"]:
                continue
            alpha = min(y_d, x_d, w_i)
            beta = (int(.01 * l * float(avg)) + int(math.log2(l))) >> 1 if l > 0 else 0
            score = f[jj] + alpha - beta
            if score > max_f:
                max_f, max_j = score, jj
                n_pred = max(0, n_pred - 1)
            elif t[jj] == i:
                n_pred += 1
                if n_pred > prm["max_pred"]:
                    break
            if p[jj] > 0:
                t[p[jj]] = i
        f[i], p[i] = max_f, max_j
        msc[i] = msc[max_j] if max_j >= 0 and msc[max_j] > max_f else max_f
    is_pred = [False] * n
    for i in range(n):
        if p[i] >= 0:
            is_pred[p[i]] = True
    run_of, k = [0] * n, 0
    for i in range(1, n):
        k += 1 if an[i][0] > an[i - 1][0] + prm["max_dist_x"] else 0
        run_of[i] = k
    starts, steps = {}, 0
    for i in range(n):
        if not is_pred[i] and msc[i] > prm["min_chain_score"]:
            j, s = i, 0
            while f[j] < msc[j]:
                j, s = p[j], s + 1
            steps = max(steps, s)
            starts[run_of[j]] = starts.get(run_of[j], 0) + 1
    return tied, max(starts.values(), default=0), steps


def fetch_seeds(ctx, arr, min_len=25):
    ctx.upload(arr[0], arr[1])
    ctx.seed_run(min_len, True, 1000)
    return ctx.seed_fetch()


@pytest.fixture(scope="module")
def repeats(tmp_path_factory):
    seq, reads = repeat_batch()
    c = Case(tmp_path_factory.mktemp("chain_diet"), [seq], ["rep"])
    arr = _arrays(reads)
    yield c, arr, oracle_text(c.oracle, arr)
    c.close()


def test_anchor_counts_at_every_path_of_the_sort_and_the_instances(repeats, monkeypatch):
    c, arr, want = repeats
    an = anchors_of(fetch_seeds(c.ctx, arr))
    counts = np.array([len(a) for a in an])
    for k in (16, 17, 64, 65, 96):
        assert (counts == k).any(), (k, sorted(set(counts.tolist())))
    assert (counts > 96).any() and (counts < 16).any()
    model = [chain_model(a) for a in an if a]
    assert sum(1 for m in model if m[0]) * 5 >= len(an), "tied sort keys in fewer than one read in five"
    assert max(m[1] for m in model) >= 2, "no run with two chain starts"
    assert max(m[2] for m in model) >= 2, "no chain end whose F < MSC walk takes more than one step"
    got, st = run(c.ctx, arr)
    same(got, want)
    monkeypatch.setenv("MONI_AF_DBG", "64")
    got_serial, _ = run(c.ctx, arr)
    same(got_serial, want)


def run_with(ctx, arr, **overrides):
    seq, offs, names, noff, q = arr
    ctx.upload(seq, offs)
    return ctx.align_run(names, noff, q, host_threads=8, **overrides)[0]


def test_the_wide_form_one_above_the_bound_of_the_predicate(repeats, monkeypatch):
    """max_dist_x = 2^28 + 1: no two anchors are too far apart (every read is one run), the predicate rejects the parameters and the general instance
    runs the 64-bit DP.  The oracle's handle takes no chaining parameters: the yardstick is the cross-check path, serial sorts and all."""
    c, arr, want = repeats
    got = run_with(c.ctx, arr, max_dist_x=NARROW_MAX_DIST + 1)
    at_bound = run_with(c.ctx, arr, max_dist_x=NARROW_MAX_DIST)              # the narrow form at the predicate's own bound
    monkeypatch.setenv("MONI_AF_DBG", "64")
    serial = run_with(c.ctx, arr, max_dist_x=NARROW_MAX_DIST + 1)
    serial_at_bound = run_with(c.ctx, arr, max_dist_x=NARROW_MAX_DIST)
    same(got, serial)
    same(at_bound, serial_at_bound)
    same(at_bound, got)                                                      # (no reference end of this index is 2^28 from another: the two parameters chain alike)


def test_the_early_exits_of_the_predecessor_loop(repeats, monkeypatch):
    """max_pred = 1 and max_iter = 3: the loop over the predecessors ends at its bounds for most anchors of a repeat-rich read"""
    c, arr, want = repeats
    an = anchors_of(fetch_seeds(c.ctx, arr))
    assert sum(1 for a in an if len(a) > 16) >= 100          # (anchors with more than three predecessors in reach: the repeats' copies end at the same offsets)
    got = run_with(c.ctx, arr, max_pred=1, max_iter=3)
    monkeypatch.setenv("MONI_AF_DBG", "64")
    serial = run_with(c.ctx, arr, max_pred=1, max_iter=3)
    same(got, serial)


def test_pairs_of_more_than_64_anchors_with_secondary_chains():
    """-Z: the second track (f2 / p2 / t2) of the chaining DP, on a 12-haplotype index: a mate's seeds have about 12 occurrences each"""
    from moni_align_amd import capi, index_build, synth
    from oracle import orc
    from tests.test_gpu_pe import gpu_align_all
    from tests.test_host_sim_pe import first_diff, interleave, oracle_pe
    from tests.test_oracle_pe import make_pairs
    pg = synth.make_pangenome(20000, 12, site_spacing=300)
    fi = index_build.build_from_pangenome(pg, device="cpu")
    o = orc.OracleIndex(fi=fi)
    m1, m2, _ = make_pairs(pg, 300, seed=5)
    want, st = oracle_pe(o, m1, m2, b_size=512, find_orphan=True, secondary_chains=True)
    seq, offs, names, noff, q = interleave(m1, m2)
    idx = capi.Index(fi=fi)
    ctx = capi.Ctx(idx)
    try:
        counts = np.array([len(a) for a in anchors_of(fetch_seeds(ctx, (seq, offs)), dict(DEFAULTS, freq_thr=2.0))])      # (an upper bound: before the pair's own filters)
        pair = counts[0::2] + counts[1::2]
        assert (pair > 64).sum() >= 20 and (pair <= 64).any(), sorted(set(pair.tolist()))
        got, model, aligned = gpu_align_all(ctx, seq, offs, names, noff, q, 512, find_orphan=True, secondary_chains=1)
    finally:
        ctx.close()
        idx.close()
    assert model.mean == st["ins_mean"] and model.std_dev == st["ins_std_dev"]
    if got != want:
        raise AssertionError("SAM differs at record %d:\n got: %s\nwant: %s" % first_diff(got, want))


def test_reads_of_more_anchors_than_the_large_instance_holds(tmp_path, monkeypatch):
    """a segment in 90 copies: a read of three seeds or more has more than 256 anchors (the large instance holds 256) and fewer than 2048 (the huge one's),
    so classify_kernel lists it for the huge instance, and no read of the batch is handed to align_kernel for its anchors"""
    from moni_align_amd import synth
    rng = np.random.default_rng(11)
    seg = ACGT[rng.integers(0, 4, size=SEG)]
    seq = np.concatenate([np.concatenate([seg, ACGT[rng.integers(0, 4, size=GAP)]]) for _ in range(90)])
    reads = []
    for k in range(120):
        p = int(rng.integers(0, SEG - READ))
        r = _sub(seg[p:p + READ], [int(v) for v in rng.choice(READ, size=1 + k % 4, replace=False)])
        reads.append(r if rng.random() < 0.5 else synth.revcomp(r[None, :])[0].copy())
    c = Case(tmp_path, [seq], ["rep90"])
    try:
        arr = _arrays(reads)
        want = oracle_text(c.oracle, arr)
        counts = np.array([len(a) for a in anchors_of(fetch_seeds(c.ctx, arr))])
        assert ((counts > 256) & (counts <= 2048)).sum() >= 20 and counts.max() <= 2048, sorted(set(counts.tolist()))
        got, st = run(c.ctx, arr)
        same(got, want)
        assert "anchors" not in st["handover_why"] and "long_read" not in st["handover_why"], st
        monkeypatch.setenv("MONI_AF_DBG", "64")          # the general form of the huge instance
        got_serial, _ = run(c.ctx, arr)
        same(got_serial, want)
    finally:
        c.close()
