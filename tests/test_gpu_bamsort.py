"""The coordinate sort of BAM records on the GPU: Ctx.bam_sort(raw=True) gives, byte for byte, the records, keys' order, offsets and index entries of
the host replay of the same per-record code (tests/test_host_bamsort.py) on every input of that file; the compressed form is moni_bgzf_compress of
those bytes; moni_bam_sorted_run of SAM text is the model's sort of the model's encoding; neither depends on the call or the context; bad records
are refused with the replay's counts; the context's other state is left alone."""
import ctypes as C
import threading

import numpy as np
import pytest

from tests import bam_model as bam
from tests import bamsort_model as bsm
from tests import bgzf_model as bm
from tests import test_host_bamsort as hs
from tests.bamsort_cases import BAD, H1, H2, REASONS, bad_batch, offsets
from tests.test_bam_model import SAMS, golden

pytestmark = pytest.mark.gpu

EINVAL = -22


@pytest.fixture(scope="module")
def rig(small_case):
    from moni_align_amd import capi
    idx = capi.Index(fi=small_case.fi, device=0)
    ctx = capi.Ctx(idx)
    yield capi, idx, ctx
    ctx.close()
    idx.close()


def check(ctx, header, recs):
    rc, want, wkeys, woff, wents, _ = hs.sim_sort(header, b"".join(recs), offsets(recs))
    assert rc == 0
    ctx.bam_set_header(header)
    raw, ents, st = ctx.bam_sort(b"".join(recs), offsets(recs), raw=True)
    assert raw == want, "the kernels' records differ from the host replay's (%d and %d bytes)" % (len(raw), len(want))
    assert np.array_equal(ents, wents) and ents["off"].tolist() == woff[:-1].tolist()
    assert (st["in_bytes"], st["records"], st["bam_bytes"], st["out_bytes"], st["blocks"]) == (len(want), len(recs), len(want), len(want), 0)
    assert (st["bad_records"], st["first_bad_record"], st["bad_reason"]) == (0, 0, 0)
    assert st["t_total"] >= st["t_key"] + st["t_sort"] + st["t_gather"] >= 0 and st["t_deflate"] == 0 and (not recs or st["t_gather"] > 0)
    for eof in (False, True):
        z, e2, zst = ctx.bam_sort(b"".join(recs), offsets(recs), eof=eof)
        assert z == ctx.bgzf_compress(want, eof=eof)[0], "the blocks differ from moni_bgzf_compress's of the same bytes"
        assert b"".join(b for b, _ in bm.walk(z)) == want and np.array_equal(e2, wents)
        assert zst["out_bytes"] == len(z) and zst["blocks"] == (len(want) + 65279) // 65280 + eof and zst["bam_bytes"] == len(want)
    return raw, wkeys, woff


@pytest.mark.parametrize("case", hs.CASES, ids=[c[0] for c in hs.CASES])
def test_sort_equals_host_replay(rig, case):
    _, header, recs = case
    check(rig[2], header, recs)


@pytest.mark.parametrize("name", SAMS)
def test_sorted_run_of_sam_text(rig, name):
    ctx = rig[2]
    header, lines = golden(name)
    ctx.bam_set_header(header)
    n_ref = len(bam.references(header))
    want = bsm.sort_list(n_ref, bsm.split_records(bam.encode_records(header, lines)))
    rec, keys, offs, st = ctx.bam_sorted_run(lines)
    assert rec == b"".join(want) and keys.tolist() == [bsm.key(n_ref, r) for r in want] and offs.tolist() == offsets(want).tolist()
    assert (st["records"], st["bam_bytes"], st["in_bytes"]) == (len(want), len(rec), len(lines)) and st["t_encode"] > 0 and st["t_total"] >= st["t_encode"]
    assert ctx.bam_records(lines, raw=True)[0] == bam.encode_records(header, lines)          # the encoder still answers as before
    assert ctx.bam_sorted_run(lines)[0] == rec
    # a run cut between lines, sorted again as one chunk, is the whole run: what the front end's second phase relies on
    cut = len(b"".join(lines.splitlines(keepends=True)[:len(want) // 3]))
    a, b = ctx.bam_sorted_run(lines[:cut]), ctx.bam_sorted_run(lines[cut:])
    assert ctx.bam_sort(a[0] + b[0], np.concatenate([a[2], b[2][1:] + a[2][-1]]), raw=True)[0] == rec


def test_empty_and_bad_lines(rig):
    capi, _, ctx = rig
    ctx.bam_set_header(H2)
    rec, keys, offs, st = ctx.bam_sorted_run(b"")
    assert rec == b"" and keys.size == 0 and offs.tolist() == [0] and st["records"] == 0
    for kw, want in ((dict(raw=True), b""), (dict(), b""), (dict(eof=True), bm.EOF_BLOCK)):
        out, ents, st = ctx.bam_sort(b"", np.zeros(1, np.uint64), **kw)
        assert out == want and ents.size == 0 and st["records"] == 0
    from tests import test_host_bam as hb
    ctx.bam_set_header(hb.HEADER)
    text = hb.bad_text(hb.BAD[3][1], 2, hb.BAD[0][1], 8)
    want = hb.sim_records(hb.HEADER, text)[2]
    with pytest.raises(capi.BamBadLine) as e:
        ctx.bam_sorted_run(text)
    assert (e.value.stats["bad_lines"], e.value.stats["first_bad_line"], e.value.stats["bad_reason"]) == (want["bad_lines"], want["first_bad_line"], want["bad_reason"])
    with pytest.raises(capi.BamBadLine):
        ctx.bam_sorted_run(hb.GOOD_LINES[0][:-1])


def test_two_contexts_two_threads(rig):
    capi, idx, _ = rig
    by = {c[0]: c for c in hs.CASES}
    inputs = [by["random2000"], by["refs_300"]]
    want = [hs.sim_sort(h, b"".join(r), offsets(r))[1] for _, h, r in inputs]
    got, errs = [None, None], []

    def work(k):
        try:
            ctx = capi.Ctx(idx)
            try:
                _, h, recs = inputs[k]
                ctx.bam_set_header(h)
                for _ in range(3):
                    got[k] = ctx.bam_sort(b"".join(recs), offsets(recs), raw=True)[0]
                    assert got[k] == want[k]
                    assert b"".join(b for b, _ in bm.walk(ctx.bam_sort(b"".join(recs), offsets(recs), block_size=4096, eof=True)[0], 4096)) == want[k]
            finally:
                ctx.close()
        except BaseException as e:          # noqa: B036 - handed to the main thread
            errs.append(e)

    ts = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    assert got == want


def test_align_state_is_left_alone(rig, small_case):
    """the SAM text of an align_batch is sorted; the batch, the counters, the kernel times and a pending fetch stay"""
    capi, idx, ctx = rig
    synth = small_case.synth
    reads = synth.make_reads(small_case.pg, 300, 150, seed=5)
    offs = np.arange(0, (len(reads) + 1) * 150, 150, dtype=np.uint64)
    names, noff = synth.make_names(len(reads))
    quals = np.full(reads.size, ord("I"), dtype=np.uint8)
    sam, st = ctx.align_batch(reads.reshape(-1), offs, names, noff, quals, host_threads=2, stream=True)
    assert st["aligned"] > 0
    header = ctx.sam_header()
    ctx.bam_set_header(header)

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
    rec, keys, roff, _ = ctx.bam_sorted_run(sam)
    assert rec == bsm.sort(header, bam.encode_records(header, sam)) and (np.diff(keys.astype(np.int64)) >= 0).all()
    z, ents, _ = ctx.bam_sort(rec, roff, eof=True)
    assert b"".join(b for b, _ in bm.walk(z)) == rec and ents["off"].tolist() == roff[:-1].tolist()
    assert state() == before
    sam2, st2 = ctx.align_batch(reads.reshape(-1), offs, names, noff, quals, host_threads=2, stream=True)
    assert sam2 == sam and st2["aligned"] == st["aligned"]
    ctx.upload(reads.reshape(-1), offs)
    ctx.screen_run()
    ctx.bam_sorted_run(sam)
    ctx.bam_sort(rec, roff)
    res = ctx.screen_fetch()
    assert len(res) == len(reads) and np.array_equal(res, ctx.screen_batch(reads.reshape(-1), offs))


@pytest.mark.parametrize("case", BAD, ids=[b[0] for b in BAD])
def test_bad_records(rig, case):
    capi, _, ctx = rig
    ctx.bam_set_header(H1)
    for rec, off in (bad_batch(case), bad_batch(case, 0), bad_batch(case, 9), bad_batch(case, 2, BAD[3], 8), bad_batch(BAD[4], 1, case, 9)):
        want = hs.sim_sort(H1, rec, off)
        assert want[0] == EINVAL
        with pytest.raises(capi.BamBadRecord) as e:
            ctx.bam_sort(rec, off, raw=True)
        st = e.value.stats
        if int(off[-1]) != len(rec):          # the last record's end is its start: offs[n] is not len, which the call sees before any record
            assert (st["bad_records"], st["first_bad_record"], st["bad_reason"]) == (1, len(off) - 1, REASONS.index("LENGTH"))
        else:
            assert (st["bad_records"], st["first_bad_record"], st["bad_reason"]) == (want[5]["bad_records"], want[5]["first_bad_record"], want[5]["bad_reason"])
        assert st["out_bytes"] == 0 and st["bam_bytes"] == 0
    assert hs.sim_sort(H1, *bad_batch(case))[5]["bad_reason"] == REASONS.index(case[2])


def test_errors(rig):
    capi, idx, ctx = rig
    L = capi.lib()
    recs = hs.CASES[3][2]          # n63
    data, off = b"".join(recs), offsets(recs)
    buf = C.create_string_buffer(data, len(data))
    out, n, ents, st = C.c_void_p(), C.c_uint64(5), C.c_void_p(), capi.BamSortStatsC()
    good = capi.BamParamsC()
    L.moni_bam_params_default(C.byref(good))

    def call(h, d, ln, o, cnt, p, po=C.byref(out), pn=C.byref(n), pe=C.byref(ents)):
        return L.moni_bam_sort(h, d, ln, o, cnt, p, po, pn, pe, C.byref(st))

    fresh = capi.Ctx(idx)          # before a header is set
    try:
        assert L.moni_bam_sort(fresh._h, buf, len(data), off.ctypes.data, len(recs), C.byref(good), C.byref(out), C.byref(n), C.byref(ents), C.byref(st)) == EINVAL
        with pytest.raises(RuntimeError, match="-22"):
            fresh.bam_sorted_run(b"")
        fresh.bam_set_header(H2)
        assert fresh.bam_sort(data, off, raw=True)[0] == hs.sim_sort(H2, data, off)[1]
    finally:
        fresh.close()
    ctx.bam_set_header(H2)
    assert call(ctx._h, buf, len(data), off.ctypes.data, len(recs), C.byref(good)) == 0 and n.value > 0
    assert call(None, buf, len(data), off.ctypes.data, len(recs), C.byref(good)) == EINVAL
    assert call(ctx._h, None, len(data), off.ctypes.data, len(recs), C.byref(good)) == EINVAL
    assert call(ctx._h, buf, len(data), None, len(recs), C.byref(good)) == EINVAL
    assert call(ctx._h, buf, len(data), off.ctypes.data, len(recs), None) == EINVAL
    assert call(ctx._h, buf, len(data), off.ctypes.data, len(recs), C.byref(good), po=None) == EINVAL
    assert call(ctx._h, buf, len(data), off.ctypes.data, len(recs), C.byref(good), pn=None) == EINVAL
    assert call(ctx._h, buf, len(data), off.ctypes.data, len(recs), C.byref(good), pe=None) == EINVAL
    for kw in (dict(block_size=0), dict(block_size=65281), dict(level=2), dict(eof=2), dict(raw=2)):
        p = capi.BamParamsC(65280, 1, 0, 0)
        for k, v in kw.items():
            setattr(p, k, v)
        assert call(ctx._h, buf, len(data), off.ctypes.data, len(recs), C.byref(p)) == EINVAL, kw
    p = capi.BamParamsC(65280, 1, 0, 0)
    p.reserved[1] = 1
    assert call(ctx._h, buf, len(data), off.ctypes.data, len(recs), C.byref(p)) == EINVAL
    # offs[n] is not len: nothing is written, the records are not looked at
    n.value = 5
    assert call(ctx._h, buf, len(data) - 1, off.ctypes.data, len(recs), C.byref(good)) == EINVAL and n.value == 0
    assert (st.bad_records, st.first_bad_record, st.bad_reason) == (1, len(recs), REASONS.index("LENGTH"))
    check(ctx, H2, recs)
