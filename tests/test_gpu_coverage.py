"""Depth of coverage on the GPU (moni_cov_*) against tests/coverage_model on the cases of tests/coverage_cases: the stats of an
add, the figures of the seal, the per-base text at every window of the grid, the window sums; moni_cov_add_sorted against moni_cov_add of
the bytes the sort returned; two contexts adding from two threads; every refusal; the 2^31 bound through the test seam; and what a context
held before is left alone."""
import ctypes as C
import threading

import numpy as np
import pytest

from tests import bamsort_model as bsm
from tests import coverage_model as cm
from tests.bamsort_cases import BAD, GOOD, REASONS, bad_batch, offsets
from tests.coverage_cases import BASES_GRID, H_ONE, HDR, LINES_GRID, WINDOWS, cases

pytestmark = pytest.mark.gpu

EINVAL, ERANGE = -22, -34
CASES = cases()
MODELS = {name: cm.Coverage(HDR, min_mapq=q).add(recs) for name, recs, q in CASES}          # computed once, read by every test
STAT_KEYS = ("records", "counted", "skipped_flag", "skipped_mapq", "unplaced", "clipped", "blocks", "bad_records", "first_bad_record", "bad_reason")


@pytest.fixture(scope="module")
def rig(small_case):
    from moni_align_amd import capi
    idx = capi.Index(fi=small_case.fi, device=0)
    ctx = capi.Ctx(idx)
    yield capi, idx, ctx
    ctx.close()
    idx.close()


def case(name):
    return next(c for c in CASES if c[0] == name)


def figures(st):
    return {k: st[k] for k in STAT_KEYS}


def model_stats(m):
    return dict(m.stats, bad_records=0, first_bad_record=0, bad_reason=0)


def pieces(cov, ctx, mb, ml):
    out = []
    for _ in range(100000):
        rc, piece, done = cov.next(ctx, mb, ml)
        assert rc == 0 and piece.count(b"\n") <= ml and (not piece or piece.endswith(b"\n"))
        out.append(piece)
        if done:
            return b"".join(out)
    raise AssertionError("moni_cov_next does not end")


@pytest.mark.parametrize("name,recs,mapq", CASES, ids=[c[0] for c in CASES])
def test_abi_matches_model(rig, name, recs, mapq):
    capi, _, ctx = rig
    ctx.bam_set_header(HDR)
    m = MODELS[name]
    cov = capi.Coverage(ctx, min_mapq=mapq)
    try:
        rc, st = cov.add(ctx, b"".join(recs), offsets(recs))
        assert rc == 0 and figures(st) == model_stats(m) and st["t_total"] >= 0 and (not recs or st["t_add"] > 0)
        rc, refs = cov.seal(ctx)
        assert rc == 0 and refs == m.ref_figures()
        assert cov.seal(ctx) == (0, refs), "a second seal"
        assert cov.add(ctx, b"".join(recs), offsets(recs))[0] == EINVAL, "an add after the seal"
        assert pieces(cov, ctx, 1 << 20, 1 << 20) == m.per_base()
        assert cov.next(ctx, 7, 2) == (0, b"", 1), "behind the last piece"
        for r in range(3):
            for w in WINDOWS:
                assert cov.windows(ctx, r, w) == (0, m.windows(r, w)), (r, w)
    finally:
        cov.close()


@pytest.mark.parametrize("name", ["edges", "cigars", "pile257", "boundary", "empty_ref", "random3000"])
def test_text_is_the_same_at_every_window(rig, name):
    capi, _, ctx = rig
    ctx.bam_set_header(HDR)
    _, recs, mapq = case(name)
    want = MODELS[name].per_base()
    for mb, ml in [(mb, ml) for mb in BASES_GRID for ml in LINES_GRID]:
        cov = capi.Coverage(ctx, min_mapq=mapq)
        try:
            assert cov.add(ctx, b"".join(recs), offsets(recs))[0] == 0 and cov.seal(ctx)[0] == 0
            assert pieces(cov, ctx, mb, ml) == want, (mb, ml)
        finally:
            cov.close()


def test_add_sorted_equals_add_of_the_returned_bytes(rig):
    capi, _, ctx = rig
    ctx.bam_set_header(HDR)
    _, recs, _ = case("random3000")
    rng = np.random.default_rng(3)
    marks = (rng.random(len(recs)) < 0.2).astype(np.uint8)
    a, b, plain = capi.Coverage(ctx), capi.Coverage(ctx), capi.Coverage(ctx)
    try:
        raw, ents, _ = ctx.bam_sort_marked(b"".join(recs), offsets(recs), marks, raw=True)
        out = bsm.split_records(raw)
        assert sum(1 for r in out if r[19] & 4) >= int(marks.sum()) > 0
        rc, st = a.add_sorted(ctx)
        rc2, st2 = b.add(ctx, raw, offsets(out))
        assert rc == 0 and rc2 == 0 and figures(st) == figures(st2)
        want = cm.Coverage(HDR).add(out)
        assert figures(st) == model_stats(want)
        assert a.seal(ctx)[1] == b.seal(ctx)[1] == want.ref_figures()
        assert a.text(ctx, 64, 1000) == b.text(ctx) == want.per_base()
        plain.add(ctx, b"".join(recs), offsets(recs))
        plain.seal(ctx)
        assert plain.text(ctx) != want.per_base(), "the marks of the sort change the depth"
        # behind a deflated sort and behind an empty one
        ctx.bam_sort(b"".join(recs[:100]), offsets(recs[:100]))
        c = capi.Coverage(ctx)
        assert c.add_sorted(ctx)[0] == 0 and c.seal(ctx)[1] == cm.Coverage(HDR).add(recs[:100]).ref_figures()
        c.close()
        ctx.bam_sort(b"", offsets([]))
        c = capi.Coverage(ctx)
        assert c.add_sorted(ctx)[1]["records"] == 0
        c.close()
    finally:
        for x in (a, b, plain):
            x.close()


def test_sorted_run_then_add_sorted(rig):
    capi, _, ctx = rig
    from tests.test_bam_model import golden
    header, lines = golden("align_small.sam")
    ctx.bam_set_header(header)
    rec, keys, offs, _ = ctx.bam_sorted_run(lines)
    cov = capi.Coverage(ctx)
    try:
        rc, st = cov.add_sorted(ctx)
        want = cm.Coverage(header).add(bsm.split_records(rec))
        assert rc == 0 and figures(st) == model_stats(want) and st["counted"] > 0
        assert cov.seal(ctx)[1] == want.ref_figures() and cov.text(ctx, 1000, 50) == want.per_base()
    finally:
        cov.close()


def test_two_contexts_two_threads(rig):
    capi, idx, ctx = rig
    ctx.bam_set_header(HDR)
    other = capi.Ctx(idx)
    other.bam_set_header(HDR)
    _, recs, _ = case("random3000")
    cov = capi.Coverage(ctx)
    got, errs = {}, []

    def work(cx, part, key):
        try:
            for lo in range(0, len(part), 500):
                rc, st = cov.add(cx, b"".join(part[lo:lo + 500]), offsets(part[lo:lo + 500]))
                assert rc == 0
                got[key] = got.get(key, 0) + st["counted"]
        except Exception as e:          # noqa: BLE001
            errs.append(e)

    try:
        th = [threading.Thread(target=work, args=(ctx, recs[:1500], 0)), threading.Thread(target=work, args=(other, recs[1500:], 1))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        m = MODELS["random3000"]
        assert got[0] + got[1] == m.stats["counted"]
        assert cov.seal(other)[1] == m.ref_figures() and cov.text(other, 64, 3) == m.per_base()
    finally:
        cov.close()
        other.close()


def test_refusals(rig):
    capi, idx, ctx = rig
    bare = capi.Ctx(idx)
    try:
        with pytest.raises(ValueError, match="-22"):
            capi.Coverage(bare)          # no header
        ctx.bam_set_header(HDR)
        with pytest.raises(ValueError, match="-22"):
            capi.Coverage(ctx, reserved=(0, 1))
        with pytest.raises(ValueError, match="-22"):
            capi.Coverage(ctx, reserved=(1, 0))
        cov = capi.Coverage(ctx)
        assert cov.next(ctx, 1, 1)[0] == EINVAL and cov.windows(ctx, 0, 1)[0] == EINVAL, "before the seal"
        bare.bam_set_header(HDR)
        assert cov.add_sorted(bare)[0] == EINVAL, "no sort has run on that context"
        bare.bam_set_header(H_ONE)
        assert cov.add(bare, b"".join(GOOD), offsets(GOOD))[0] == EINVAL, "a context with another dictionary"
        assert cov.add(ctx, b"".join(GOOD) + b"x", offsets(GOOD))[1]["bad_reason"] == REASONS.index("LENGTH")
        assert cov.seal(ctx)[0] == 0
        assert cov.add(ctx, b"", offsets([]))[0] == EINVAL and cov.add_sorted(ctx)[0] == EINVAL, "after the seal"
        assert cov.next(ctx, 0, 1)[0] == EINVAL and cov.next(ctx, 1, 0)[0] == EINVAL
        assert cov.windows(ctx, 3, 1)[0] == EINVAL and cov.windows(ctx, 0, 0)[0] == EINVAL and cov.windows(ctx, 0, 1 << 31)[0] == EINVAL
        assert cov.text(ctx) == b"a\t0\t1\t0\nchrB\t0\t70\t0\nc\t0\t200\t0\n"
        cov.close()
    finally:
        bare.close()


@pytest.mark.parametrize("bad", BAD, ids=[b[0] for b in BAD])
def test_bad_record_adds_nothing(rig, bad):
    capi, _, ctx = rig
    ctx.bam_set_header(H_ONE)
    cov = capi.Coverage(ctx)
    try:
        data, off = bad_batch(bad)
        rc, st = cov.add(ctx, data, off)
        assert rc == EINVAL and st["bad_records"] >= 1 and st["first_bad_record"] == 5 and REASONS[st["bad_reason"]] == bad[2]
        data2, off2 = bad_batch(bad, at=6, second=BAD[3], second_at=2)
        rc, st = cov.add(ctx, data2, off2)
        assert rc == EINVAL and st["first_bad_record"] == 2 and REASONS[st["bad_reason"]] == BAD[3][2], "the lowest index"
        assert cov.add(ctx, b"".join(GOOD[:2]), offsets(GOOD[:2]))[1]["counted"] == 2
        assert cov.seal(ctx)[1] == cm.Coverage(H_ONE).add(GOOD[:2]).ref_figures(), "nothing of the bad calls was added"
    finally:
        cov.close()


def test_limit_through_the_seam(rig):
    capi, _, ctx = rig
    ctx.bam_set_header(HDR)
    _, recs, _ = case("pile65")
    cov = capi.Coverage(ctx)
    try:
        cov.test_set_counted(cm.LIMIT - 66)
        assert cov.add(ctx, b"".join(recs), offsets(recs))[0] == 0, "2^31 - 1 counted records"
        assert cov.add(ctx, recs[0], offsets(recs[:1]))[0] == ERANGE
        ctx.bam_sort(b"".join(recs[:3]), offsets(recs[:3]), raw=True)
        assert cov.add_sorted(ctx)[0] == ERANGE
        tail = case("cigars")[1][-3:]
        assert cov.add(ctx, b"".join(tail), offsets(tail))[0] == 0, "records that do not count still pass"
        assert cov.seal(ctx)[1] == MODELS["pile65"].ref_figures(), "the refused calls added nothing"
    finally:
        cov.close()


def test_context_state_is_left_alone(rig, small_case):
    """the resident batch, a pending fetch, the kernel times and the counters survive the coverage calls, and so do the sort's results"""
    capi, _, ctx = rig
    synth = small_case.synth
    reads = synth.make_reads(small_case.pg, 300, 150, seed=5)
    offs = np.arange(0, (len(reads) + 1) * 150, 150, dtype=np.uint64)
    ctx.upload(reads.reshape(-1), offs)
    ctx.ms_run()
    ctx.screen_run()
    ctx.bam_set_header(HDR)
    _, recs, _ = case("random3000")
    raw, ents, _ = ctx.bam_sort(b"".join(recs), offsets(recs), raw=True)

    def state():
        ms = {}
        for which in range(7):
            try:
                ms[which] = ctx.kernel_ms(which)
            except RuntimeError:          # that stage did not run
                pass
        return ms, ctx.counters().tolist()

    before = state()
    assert before[0]
    cov = capi.Coverage(ctx)
    try:
        assert cov.add_sorted(ctx)[0] == 0 and cov.add(ctx, b"".join(recs[:50]), offsets(recs[:50]))[0] == 0
        assert cov.seal(ctx)[0] == 0 and cov.text(ctx, 64, 3) and cov.windows(ctx, 2, 16)[0] == 0
    finally:
        cov.close()
    after = state()
    # Two reads of one pair of events need not give the same float (DESIGN.md 7.16 met 0.238161996 and 0.238162994 ms): the bound is 10 ns, ten
    # ticks of the 100 MHz event clock, and the spacing of a float at these magnitudes lies below it
    assert after[1] == before[1] and after[0].keys() == before[0].keys()
    for which, ms in before[0].items():
        assert after[0][which] == pytest.approx(ms, rel=1e-6, abs=1e-5)
    raw2, ents2, _ = ctx.bam_sort(b"".join(recs), offsets(recs), raw=True)
    assert raw2 == raw and np.array_equal(ents, ents2)
    res = ctx.screen_fetch()
    assert len(res) == len(reads) and np.array_equal(res, ctx.screen_batch(reads.reshape(-1), offs))
