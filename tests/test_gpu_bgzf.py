"""The BGZF writer on the GPU: Ctx.bgzf_compress gives, byte for byte, what the host replay of the same per-block code gives
(tests/test_host_bgzf.py), for every input of that file; the stream does not depend on the call, the context or the cut of the input."""
import ctypes as C
import gzip
import threading

import numpy as np
import pytest

from tests import bgzf_model as bm
from tests import test_host_bgzf as hb

pytestmark = pytest.mark.gpu

EINVAL = -22
COUNTS = ("in_bytes", "out_bytes", "blocks", "stored_blocks", "matches", "literals")


@pytest.fixture(scope="module")
def rig(small_case):
    from moni_align_amd import capi
    idx = capi.Index(fi=small_case.fi, device=0)
    ctx = capi.Ctx(idx)
    yield capi, idx, ctx
    ctx.close()
    idx.close()


def check(ctx, data, bs=65280, level=1, eof=False):
    z, st = ctx.bgzf_compress(data, block_size=bs, level=level, eof=eof)
    want, wst = hb.sim_compress(data, bs, level, eof)
    assert z == want, "the kernel's stream differs from the host replay's (%d and %d bytes)" % (len(z), len(want))
    assert {k: st[k] for k in COUNTS} == {k: wst[k] for k in COUNTS}
    blocks = bm.walk(z, bs)
    assert b"".join(b for b, _ in blocks) == data
    nb = (len(data) + bs - 1) // bs
    assert st["blocks"] == len(blocks) and st["in_bytes"] == len(data) and st["out_bytes"] == len(z)
    assert st["stored_blocks"] == sum(1 for _, t in blocks[:nb] if t == 0)
    assert st["t_total"] >= st["t_kernel"] >= 0
    return z, st


@pytest.mark.parametrize("case", hb.CASES, ids=[c[0] for c in hb.CASES])
def test_stream_equals_host_replay(rig, case):
    _, data, bs, level, eof = case
    check(rig[2], data, bs, level, eof)


def test_repeat_and_eof(rig):
    ctx = rig[2]
    data = hb.golden("pe_small.sam")
    a, _ = check(ctx, data, eof=False)
    b, st = check(ctx, data, eof=True)
    c, _ = ctx.bgzf_compress(data, eof=True)
    assert b == c == a + bm.EOF_BLOCK and not a.endswith(bm.EOF_BLOCK)
    assert gzip.decompress(b) == data
    z, st = ctx.bgzf_compress(b"")
    assert z == b"" and all(st[k] == 0 for k in COUNTS) and st["t_kernel"] == 0
    z, st = ctx.bgzf_compress(b"", eof=True)
    assert z == bm.EOF_BLOCK and st["blocks"] == 1 and st["out_bytes"] == 28


def test_split_at_block_boundaries(rig):
    ctx = rig[2]
    data = hb.golden("pe_small_orphan.sam")
    for bs, cut in ((65280, 65280), (4096, 5 * 4096), (258, 100 * 258)):
        whole, _ = ctx.bgzf_compress(data, block_size=bs)
        a, _ = ctx.bgzf_compress(data[:cut], block_size=bs)
        b, _ = ctx.bgzf_compress(data[cut:], block_size=bs)
        assert whole == a + b


def test_two_contexts_two_threads(rig):
    capi, idx, _ = rig
    inputs = [hb.golden("pe_small.sam"), hb.golden("pe_small_orphan.sam")]
    want = [hb.sim_compress(d, 4096, 1, True)[0] for d in inputs]
    got, errs = [None, None], []

    def work(k):
        try:
            ctx = capi.Ctx(idx)
            try:
                for _ in range(3):
                    got[k] = ctx.bgzf_compress(inputs[k], block_size=4096, eof=True)[0]
                    assert got[k] == want[k]
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
    """the SAM text of an align_batch compresses and round-trips; the same batch aligned again gives the same text"""
    capi, idx, ctx = rig
    synth = small_case.synth
    reads = synth.make_reads(small_case.pg, 300, 150, seed=5)
    offs = np.arange(0, (len(reads) + 1) * 150, 150, dtype=np.uint64)
    names, noff = synth.make_names(len(reads))
    quals = np.full(reads.size, ord("I"), dtype=np.uint8)
    sam, st = ctx.align_batch(reads.reshape(-1), offs, names, noff, quals, host_threads=2, stream=True)
    assert st["aligned"] > 0 and len(sam) > 30000
    z, bst = check(ctx, sam, eof=True)
    assert gzip.decompress(z) == sam and len(z) < len(sam) // 2
    z2, _ = check(ctx, sam, bs=4096)
    assert gzip.decompress(z2) == sam
    sam2, st2 = ctx.align_batch(reads.reshape(-1), offs, names, noff, quals, host_threads=2, stream=True)
    assert sam2 == sam and st2["aligned"] == st["aligned"]
    # a resident batch and a pending result survive the call
    ctx.upload(reads.reshape(-1), offs)
    ctx.screen_run()
    ctx.bgzf_compress(sam)
    res = ctx.screen_fetch()
    assert len(res) == len(reads) and np.array_equal(res, ctx.screen_batch(reads.reshape(-1), offs))


def test_errors(rig):
    capi, idx, ctx = rig
    L = capi.lib()
    data = b"ACGT" * 10
    buf = C.create_string_buffer(data)
    out, n, st = C.c_void_p(), C.c_uint64(), capi.BgzfStatsC()

    def call(h, text, ln, p, o=C.byref(out), on=C.byref(n)):
        return L.moni_bgzf_compress(h, text, ln, p, o, on, C.byref(st))

    good = capi.BgzfParamsC()
    L.moni_bgzf_params_default(C.byref(good))
    assert (good.block_size, good.level, good.eof, good.reserved) == (65280, 1, 0, 0)
    assert call(ctx._h, buf, len(data), C.byref(good)) == 0 and n.value > 0
    assert call(None, buf, len(data), C.byref(good)) == EINVAL
    assert call(ctx._h, buf, len(data), None) == EINVAL
    assert call(ctx._h, buf, len(data), C.byref(good), o=None) == EINVAL
    assert call(ctx._h, None, len(data), C.byref(good)) == EINVAL
    assert call(ctx._h, None, 0, C.byref(good)) == 0 and n.value == 0
    for kw in (dict(block_size=0), dict(block_size=65281), dict(level=2), dict(reserved=1)):
        p = capi.BgzfParamsC(65280, 1, 0, 0)
        for k, v in kw.items():
            setattr(p, k, v)
        assert call(ctx._h, buf, len(data), C.byref(p)) == EINVAL, kw
    with pytest.raises(RuntimeError, match="-22"):
        ctx.bgzf_compress(data, block_size=70000)
    # the context still works
    check(ctx, data)
