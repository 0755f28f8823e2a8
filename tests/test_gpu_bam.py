"""The BAM encoder on the GPU: Ctx.bam_records(raw=True) gives, byte for byte, what the host replay of the same per-line code gives
(tests/test_host_bam.py) for every input of that file; the compressed form is BGZF around those bytes; neither depends on the call, the
context or where the text is cut between lines; bad lines are refused with the replay's counts; the context's other state is left alone."""
import ctypes as C
import gzip
import threading

import numpy as np
import pytest

from tests import bam_model as bam
from tests import bgzf_model as bm
from tests import test_host_bam as hb

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


def check(ctx, header, lines):
    """raw bytes = the replay's; the blocks inflate to them, with and without the end-of-file block"""
    rc, want, wst = hb.sim_records(header, lines)
    assert rc == 0
    assert ctx.bam_set_header(header) == hb.sim_header(header)[1]
    raw, st = ctx.bam_records(lines, raw=True)
    assert raw == want, "the kernels' records differ from the host replay's (%d and %d bytes)" % (len(raw), len(want))
    assert (st["in_bytes"], st["lines"], st["bam_bytes"], st["out_bytes"], st["blocks"]) == (len(lines), wst["lines"], len(want), len(want), 0)
    assert (st["bad_lines"], st["first_bad_line"], st["bad_reason"]) == (0, 0, 0) and st["t_total"] >= st["t_encode"] >= 0 and st["t_deflate"] == 0
    for eof in (False, True):
        z, zst = ctx.bam_records(lines, eof=eof)
        blocks = bm.walk(z)
        assert b"".join(b for b, _ in blocks) == want and (gzip.decompress(z) if z else b"") == want
        nb = (len(want) + 65279) // 65280
        assert len(blocks) == nb + eof == zst["blocks"] and zst["out_bytes"] == len(z) and zst["bam_bytes"] == len(want)
        assert z.endswith(bm.EOF_BLOCK) == eof or not want
        assert z == ctx.bgzf_compress(want, eof=eof)[0], "the blocks differ from moni_bgzf_compress's of the same bytes"
    return raw


@pytest.mark.parametrize("case", hb.CASES, ids=[c[0] for c in hb.CASES])
def test_records_equal_host_replay(rig, case):
    _, header, lines = case
    check(rig[2], header, lines)


def test_small_blocks_repeat_and_empty(rig):
    ctx = rig[2]
    header, lines = hb.golden("pe_small.sam")
    raw = check(ctx, header, lines)
    z, st = ctx.bam_records(lines, block_size=4096, eof=True)
    assert b"".join(b for b, _ in bm.walk(z, 4096)) == raw and st["blocks"] == (len(raw) + 4095) // 4096 + 1
    assert ctx.bam_records(lines, block_size=4096, eof=True)[0] == z and ctx.bam_records(lines, raw=True)[0] == raw
    assert ctx.bam_records(lines, level=0)[1]["out_bytes"] == len(raw) + 31 * ((len(raw) + 65279) // 65280)
    for kw, want in ((dict(), b""), (dict(eof=True), bm.EOF_BLOCK), (dict(raw=True), b""), (dict(raw=True, eof=True), b"")):
        z, st = ctx.bam_records(b"", **kw)
        assert z == want and (st["lines"], st["bam_bytes"], st["out_bytes"], st["blocks"]) == (0, 0, len(want), len(want) // 28)


def test_cut_between_lines(rig):
    ctx = rig[2]
    header, lines = hb.golden("pe_small_orphan.sam")
    ctx.bam_set_header(header)
    whole = ctx.bam_records(lines, raw=True)[0]
    for cut in (1, 160, 319):
        at = len(b"".join(lines.splitlines(keepends=True)[:cut]))
        assert ctx.bam_records(lines[:at], raw=True)[0] + ctx.bam_records(lines[at:], raw=True)[0] == whole


def test_two_contexts_two_threads(rig):
    capi, idx, _ = rig
    inputs = [hb.golden("pe_small.sam"), (hb.HEADER, b"".join(hb.random_lines(500, 23)))]
    want = [hb.sim_records(h, t)[1] for h, t in inputs]
    got, errs = [None, None], []

    def work(k):
        try:
            ctx = capi.Ctx(idx)
            try:
                ctx.bam_set_header(inputs[k][0])
                for _ in range(3):
                    got[k] = ctx.bam_records(inputs[k][1], raw=True)[0]
                    assert got[k] == want[k]
                    assert gzip.decompress(ctx.bam_records(inputs[k][1], block_size=4096, eof=True)[0]) == want[k]
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
    """the SAM text of an align_batch goes through and reads back; the batch, the counters, the kernel time and a pending fetch stay"""
    capi, idx, ctx = rig
    synth = small_case.synth
    reads = synth.make_reads(small_case.pg, 300, 150, seed=5)
    offs = np.arange(0, (len(reads) + 1) * 150, 150, dtype=np.uint64)
    names, noff = synth.make_names(len(reads))
    quals = np.full(reads.size, ord("I"), dtype=np.uint8)
    sam, st = ctx.align_batch(reads.reshape(-1), offs, names, noff, quals, host_threads=2, stream=True)
    assert st["aligned"] > 0 and len(sam) > 30000
    header = ctx.sam_header()
    bh = ctx.bam_set_header(header)
    assert bh == bam.encode_header(header)

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
    z, bst = ctx.bam_records(sam, eof=True)
    assert bst["lines"] == sam.count(b"\n") and bam.decode(bh + gzip.decompress(z)) == header + bam.canonical(sam)
    assert state() == before
    sam2, st2 = ctx.align_batch(reads.reshape(-1), offs, names, noff, quals, host_threads=2, stream=True)
    assert sam2 == sam and st2["aligned"] == st["aligned"]
    # a resident batch and a pending result survive the call
    ctx.upload(reads.reshape(-1), offs)
    ctx.screen_run()
    ctx.bam_records(sam)
    res = ctx.screen_fetch()
    assert len(res) == len(reads) and np.array_equal(res, ctx.screen_batch(reads.reshape(-1), offs))


@pytest.mark.parametrize("case", hb.BAD, ids=[b[0] for b in hb.BAD])
def test_bad_lines(rig, case):
    capi, _, ctx = rig
    _, line, reason = case
    ctx.bam_set_header(hb.HEADER)
    for text in (hb.bad_text(line), hb.bad_text(line, 2, hb.BAD[0][1], 8), hb.bad_text(hb.BAD[0][1], 1, line, 9)):
        want = hb.sim_records(hb.HEADER, text)
        assert want[0] == EINVAL
        with pytest.raises(capi.BamBadLine) as e:
            ctx.bam_records(text, raw=True)
        st = e.value.stats
        assert (st["bad_lines"], st["first_bad_line"], st["bad_reason"]) == (want[2]["bad_lines"], want[2]["first_bad_line"], want[2]["bad_reason"])
        assert st["out_bytes"] == 0 and st["bam_bytes"] == 0
    assert e.value.stats["bad_reason"] == hb.BAD[0][2] and hb.sim_records(hb.HEADER, hb.bad_text(line))[2]["bad_reason"] == reason


def test_errors(rig):
    capi, idx, ctx = rig
    L = capi.lib()
    text = hb.GOOD_LINES[0]
    buf = C.create_string_buffer(text)
    out, n, st = C.c_void_p(), C.c_uint64(5), capi.BamStatsC()

    def call(h, t, ln, p, o=C.byref(out), on=C.byref(n)):
        return L.moni_bam_records(h, t, ln, p, o, on, C.byref(st))

    good = capi.BamParamsC()
    L.moni_bam_params_default(C.byref(good))
    assert (good.block_size, good.level, good.eof, good.raw, good.reserved[0], good.reserved[1]) == (65280, 1, 0, 0, 0, 0)
    # before a header is set: a fresh context refuses
    fresh = capi.Ctx(idx)
    try:
        assert L.moni_bam_records(fresh._h, buf, len(text), C.byref(good), C.byref(out), C.byref(n), C.byref(st)) == EINVAL
        assert L.moni_bam_records(fresh._h, None, 0, C.byref(good), C.byref(out), C.byref(n), C.byref(st)) == EINVAL
        with pytest.raises(RuntimeError, match="-22"):
            fresh.bam_records(text)
        with pytest.raises(RuntimeError, match="-22"):
            fresh.bam_set_header(b"@SQ\tSN:chr1\n")
        with pytest.raises(RuntimeError, match="-22"):
            fresh.bam_records(text)
        fresh.bam_set_header(hb.HEADER)
        assert fresh.bam_records(text, raw=True)[0] == hb.sim_records(hb.HEADER, text)[1]
    finally:
        fresh.close()
    ctx.bam_set_header(hb.HEADER)
    assert call(ctx._h, buf, len(text), C.byref(good)) == 0 and n.value > 0
    assert call(None, buf, len(text), C.byref(good)) == EINVAL
    assert call(ctx._h, buf, len(text), None) == EINVAL
    assert call(ctx._h, buf, len(text), C.byref(good), o=None) == EINVAL
    assert call(ctx._h, buf, len(text), C.byref(good), on=None) == EINVAL
    assert call(ctx._h, None, len(text), C.byref(good)) == EINVAL
    assert call(ctx._h, None, 0, C.byref(good)) == 0 and n.value == 0
    for kw in (dict(block_size=0), dict(block_size=65281), dict(level=2), dict(eof=2), dict(raw=2)):
        p = capi.BamParamsC(65280, 1, 0, 0)
        for k, v in kw.items():
            setattr(p, k, v)
        assert call(ctx._h, buf, len(text), C.byref(p)) == EINVAL, kw
    for k in range(2):
        p = capi.BamParamsC(65280, 1, 0, 0)
        p.reserved[k] = 1
        assert call(ctx._h, buf, len(text), C.byref(p)) == EINVAL
    # a bad line writes nothing; the missing final newline is one
    n.value = 5
    assert call(ctx._h, buf, len(text) - 1, C.byref(good)) == EINVAL and n.value == 0
    assert (st.bad_lines, st.first_bad_line, st.bad_reason) == (1, 0, bam.NEWLINE)
    hp, hn = C.c_void_p(), C.c_uint64()
    assert L.moni_bam_set_header(None, hb.HEADER, len(hb.HEADER), C.byref(hp), C.byref(hn)) == EINVAL
    assert L.moni_bam_set_header(ctx._h, hb.HEADER, len(hb.HEADER), None, C.byref(hn)) == EINVAL
    # a refused header leaves the one that was set; the context still works
    with pytest.raises(RuntimeError, match="-22"):
        ctx.bam_set_header(b"@SQ\tSN:chr1\tLN:0\n")
    check(ctx, hb.HEADER, text)
