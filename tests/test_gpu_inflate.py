"""The BGZF reader on the GPU: Ctx.bgzf_inflate gives the text, the block counts and, for damaged streams, the member and the reason that
the host replay of the same per-member code and the model give (tests/test_host_inflate.py), for every input of that file."""
import ctypes as C
import threading

import numpy as np
import pytest

from tests import inflate_model as im
from tests import test_host_bgzf as hb
from tests import test_host_inflate as hi

pytestmark = pytest.mark.gpu

EINVAL = -22
COUNTS = ("blocks", "bad_blocks", "first_bad_block", "bad_reason", "stored", "fixed", "dynamic")


@pytest.fixture(scope="module")
def rig(small_case):
    from moni_align_amd import capi
    idx = capi.Index(fi=small_case.fi, device=0)
    ctx = capi.Ctx(idx)
    yield capi, idx, ctx
    ctx.close()
    idx.close()


def check_good(ctx, z, text, check_crc=True):
    got, st = ctx.bgzf_inflate(z, check_crc=check_crc)
    assert got == text, "the kernel's text differs (%d and %d bytes)" % (len(got), len(text))
    rc, sim_text, sim = hi.sim_inflate(z, check_crc)
    assert rc == 0 and sim_text == text and {k: st[k] for k in COUNTS} == sim
    assert st["in_bytes"] == len(z) and st["out_bytes"] == len(text) and st["t_total"] >= st["t_kernel"] >= 0
    return st


def check_bad(ctx, z, check_crc=True):
    rc, n, st = ctx.bgzf_inflate(z, check_crc=check_crc, rc_only=True)
    src, _, sim = hi.sim_inflate(z, check_crc)
    m = hi.model(z, check_crc)
    assert rc == src == EINVAL and n == 0 and st["out_bytes"] == 0
    assert {k: st[k] for k in COUNTS} == sim == {k: m[k] for k in COUNTS}
    return st


@pytest.mark.parametrize("case", hi.GOOD, ids=[c[0] for c in hi.GOOD])
def test_text_equals_original(rig, case):
    _, z, text = case
    check_good(rig[2], z, text)


@pytest.mark.parametrize("case", hi.DAMAGED, ids=[c[0] for c in hi.DAMAGED])
def test_damaged_stream(rig, case):
    _, z, reason = case
    st = check_bad(rig[2], z)
    assert (st["bad_blocks"], st["first_bad_block"], st["bad_reason"]) == (1, 0, reason)


def test_crc_flip_passes_unchecked(rig):
    z = dict((c[0], c[1]) for c in hi.DAMAGED)["crc_bit"]
    check_good(rig[2], z, hi.DAMAGED_TEXT, check_crc=False)


def test_bad_member_in_the_middle(rig):
    ctx = rig[2]
    good = im.bgzip(hi.fastq_text(3000, 5), 500)
    bad = dict((c[0], c[1]) for c in hi.DAMAGED)
    st = check_bad(ctx, good + bad["distance_before_start"] + good + bad["crc_bit"] + good)
    assert (st["bad_blocks"], st["first_bad_block"], st["bad_reason"]) == (2, 6, im.DISTANCE)
    st = check_bad(ctx, good + bad["crc_bit"] + good + b"\x1f\x8b\x08\x00" + bytes(30))
    assert (st["bad_blocks"], st["first_bad_block"], st["bad_reason"]) == (2, 6, im.CRC)
    st = check_bad(ctx, good + b"\x1f\x8b\x08\x00" + bytes(30))
    assert (st["bad_blocks"], st["first_bad_block"], st["bad_reason"]) == (1, 6, im.HEADER)
    st = check_bad(ctx, (good + good)[:-3])
    assert (st["bad_blocks"], st["first_bad_block"], st["bad_reason"]) == (1, 11, im.TRUNCATED)
    # the context still works
    check_good(ctx, good, hi.fastq_text(3000, 5))


def test_more_members_than_the_resident_grid(rig):
    """2500 members of 40 bytes pass the grid (16 workgroups per CU) only where the grid is smaller; 6000 empty members pass any"""
    name, z, text = [c for c in hi.GOOD if c[0] == "members2500"][0]
    st = check_good(rig[2], z, text)
    assert st["blocks"] == 2500
    from tests import bgzf_model as bm
    z = bm.EOF_BLOCK * 3000 + im.bgzip(text[:4000], 2) + bm.EOF_BLOCK * 1000
    got, st = rig[2].bgzf_inflate(z)
    assert got == text[:4000] and st["blocks"] == 6000 and st["fixed"] == 6000 and st["bad_blocks"] == 0


def test_two_contexts_two_threads(rig):
    capi, idx, _ = rig
    cases = [c for c in hi.GOOD if c[0] in ("fastq/level6", "bs4096")]
    got, errs = [None, None], []

    def work(k):
        try:
            ctx = capi.Ctx(idx)
            try:
                for _ in range(3):
                    got[k] = ctx.bgzf_inflate(cases[k][1])[0]
                    assert got[k] == cases[k][2]
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
    assert got == [c[2] for c in cases]


def test_round_trip_with_the_writer(rig):
    ctx = rig[2]
    sam = hb.golden("pe_small_orphan.sam")
    for bs, level in ((65280, 1), (4096, 1), (300, 0)):
        z, _ = ctx.bgzf_compress(sam, block_size=bs, level=level, eof=True)
        got, st = ctx.bgzf_inflate(z)
        assert got == sam and st["blocks"] == (len(sam) + bs - 1) // bs + 1


def test_other_results_are_left_alone(rig, small_case):
    """a pointer bgzf_compress returned, the resident batch and a pending screen_fetch survive an inflate"""
    capi, idx, ctx = rig
    L = capi.lib()
    sam = hb.golden("align_small.sam")
    buf = np.frombuffer(sam, dtype=np.uint8)
    p = capi.BgzfParamsC(65280, 1, 1, 0)
    out, n = C.c_void_p(), C.c_uint64()
    assert L.moni_bgzf_compress(ctx._h, buf.ctypes.data, buf.size, C.byref(p), C.byref(out), C.byref(n), None) == 0
    z = C.string_at(out.value, n.value)
    synth = small_case.synth
    reads = synth.make_reads(small_case.pg, 300, 150, seed=5)
    offs = np.arange(0, (len(reads) + 1) * 150, 150, dtype=np.uint64)
    ctx.upload(reads.reshape(-1), offs)
    ctx.screen_run()
    got, _ = ctx.bgzf_inflate(z)
    assert got == sam
    ctx.bgzf_inflate([c for c in hi.GOOD if c[0] == "fastq/level6"][0][1])
    assert C.string_at(out.value, n.value) == z, "the writer's buffer was touched"
    res = ctx.screen_fetch()
    assert len(res) == len(reads) and np.array_equal(res, ctx.screen_batch(reads.reshape(-1), offs))


def test_arguments(rig):
    capi, idx, ctx = rig
    L = capi.lib()
    z = im.bgzip(b"ACGT" * 10)
    buf = C.create_string_buffer(z, len(z))
    out, n, st = C.c_void_p(), C.c_uint64(), capi.InflateStatsC()

    def call(h, data, ln, p, o=C.byref(out), on=C.byref(n)):
        return L.moni_bgzf_inflate(h, data, ln, p, o, on, C.byref(st))

    good = capi.InflateParamsC()
    L.moni_inflate_params_default(C.byref(good))
    assert good.check_crc == 1 and list(good.reserved) == [0, 0, 0]
    assert call(ctx._h, buf, len(z), C.byref(good)) == 0 and n.value == 40 and C.string_at(out.value, 40) == b"ACGT" * 10
    assert call(None, buf, len(z), C.byref(good)) == EINVAL
    assert call(ctx._h, buf, len(z), None) == EINVAL
    assert call(ctx._h, buf, len(z), C.byref(good), o=None) == EINVAL
    assert call(ctx._h, buf, len(z), C.byref(good), on=None) == EINVAL
    assert call(ctx._h, None, len(z), C.byref(good)) == EINVAL
    assert call(ctx._h, None, 0, C.byref(good)) == 0 and n.value == 0 and st.blocks == 0 and st.t_kernel == 0
    assert call(ctx._h, buf, 0, C.byref(good)) == 0 and n.value == 0
    for k in range(3):
        p = capi.InflateParamsC()
        p.check_crc = 1
        p.reserved[k] = 1
        assert call(ctx._h, buf, len(z), C.byref(p)) == EINVAL
    p = capi.InflateParamsC()
    p.check_crc = 2
    assert call(ctx._h, buf, len(z), C.byref(p)) == EINVAL
    assert L.moni_bgzf_inflate(ctx._h, buf, len(z), C.byref(good), C.byref(out), C.byref(n), None) == 0 and n.value == 40
    assert ctx.bgzf_inflate(b"") == (b"", {k: 0 for k, _ in capi.InflateStatsC._fields_})
    with pytest.raises(RuntimeError, match="-22"):
        ctx.bgzf_inflate(z[:-1])
