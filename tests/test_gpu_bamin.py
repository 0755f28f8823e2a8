"""The BAM reader on the GPU: Ctx.bam_in_feed gives the texts, the counts of every call and, for damaged streams, the record and the reason that the
host replay of the same code and the model give (tests/test_host_bamin.py), for every input of tests/bamin_cases.py, fed as that file says."""
import ctypes as C
import threading

import numpy as np
import pytest

from tests import bamin_cases as bc
from tests import bamin_model as bm
from tests import inflate_model as im
from tests import test_host_bamin as hb
from tests import test_host_inflate as hi

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


def gpu_feeder(ctx, paired, member, level=1):
    """feed(data, last) as the replay has it, over `data` cut into members of `member` bytes (and the end-of-file member behind the last)"""
    def feed(data, last):
        rc, a, b, nr, st = ctx.bam_in_feed(im.bgzip(data, member, level, eof=last), paired, last, rc_only=True)
        assert st["t_total"] >= 0 and all(t >= 0 for t in st["t_kernel"].values()) and st["inflate"]["bad_blocks"] == 0
        return rc, a, b, nr, st
    return feed


def gpu_run(ctx, raw, paired, member, per_call):
    ctx.bam_in_reset()
    return hb.run_feeder(gpu_feeder(ctx, paired, member), raw, paired, member, per_call)


@pytest.mark.parametrize("case", hb.CASES, ids=[c[0] for c in hb.CASES])
def test_texts_and_counts(rig, case):
    _, raw, paired, member, per_call = case
    got = gpu_run(rig[2], raw, paired, member, per_call)
    assert got == bc.model_run(raw, paired, member, per_call)
    assert got == hb.sim_run(raw, paired, member, per_call)


@pytest.mark.parametrize("case", hb.BAD, ids=[c[0] for c in hb.BAD])
def test_damaged_stream(rig, case):
    _, raw, paired, member, per_call, index, reason = case
    got = gpu_run(rig[2], raw, paired, member, per_call)
    assert got[:3] == ("bad", index, reason)
    assert got == bc.model_run(raw, paired, member, per_call) == hb.sim_run(raw, paired, member, per_call)


def tiled(n_tiles, paired=False):
    """64 records (or 32 pairs) over and over: (raw, text1, text2) with the texts of one tile from the model"""
    tile = b"".join(bc.pair(i, 100 + i % 7, 90 + i % 5, 8) for i in range(32)) if paired else b"".join(bc.read(i, 90 + i % 21, 8, flag=0x10 if i % 5 == 0 else 4) for i in range(64))
    r = bm.Stream(paired).feed(bc.HDR + tile, True)
    return bc.HDR + tile * n_tiles, r["text1"] * n_tiles, r["text2"] * n_tiles


def test_more_segments_than_the_grid_and_than_a_group(rig):
    """6000 members of 6000 bytes: 36 MB of stream, about 1100 segments - the sweep's grid goes round, and the second group takes the chain's state from the first"""
    raw, t1, _ = tiled(6000 * 6000 // len(tiled(1)[0][len(bc.HDR):]))
    assert len(raw) > 1024 * hb.segment() + 2 * 65536
    rig[2].bam_in_reset()
    a, b, nr, st = rig[2].bam_in_feed(im.bgzip(raw, 6000, 1, eof=True), last=True)
    assert a == t1 and b == b"" and nr == st["reads"] == st["records"] == t1.count(b"\n") // 4 and st["inflate"]["blocks"] >= 6000
    assert hb.sim_run(raw, False, 65280, 0)[1] == t1
    # two calls, paired: the cut lies wherever member 1000 ends
    raw, t1, t2 = tiled(1000, True)
    z = [im.bgzip(raw[:1000 * 6000], 6000, 1), im.bgzip(raw[1000 * 6000:], 6000, 1, eof=True)]
    rig[2].bam_in_reset()
    r0, r1 = rig[2].bam_in_feed(z[0], True), rig[2].bam_in_feed(z[1], True, last=True)
    assert r0[0] + r1[0] == t1 and r0[1] + r1[1] == t2 and r0[2] + r1[2] == 1000 * 32 and r0[3]["carried_bytes"] > 0 and r1[3]["carried_bytes"] == 0


def test_two_contexts_two_threads(rig):
    capi, idx, _ = rig
    inputs = [tiled(40), tiled(30, True)]
    errs = []

    def work(k):
        try:
            ctx = capi.Ctx(idx)
            try:
                raw, t1, t2 = inputs[k]
                for _ in range(3):
                    got = gpu_run(ctx, raw, bool(k), 4096, 3)
                    assert got[0] == "ok" and got[1] == t1 and got[2] == t2
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


def test_bad_member_in_the_middle(rig):
    """the inflater's verdict comes through, and the stream is as before the call"""
    ctx = rig[2]
    raw, t1, _ = tiled(20)
    good = im.bgzip(raw, 4096)
    damaged = dict((c[0], c[1]) for c in hi.DAMAGED)
    ctx.bam_in_reset()
    a, _, nr, st = ctx.bam_in_feed(good[:len(im.bgzip(raw[:8192], 4096))])
    rc, x, y, n, bad = ctx.bam_in_feed(good + damaged["crc_bit"] + good, rc_only=True)
    assert rc == EINVAL and (x, y, n) == (b"", b"", 0) and bad["bad_records"] == 0
    assert (bad["inflate"]["bad_blocks"], bad["inflate"]["first_bad_block"], bad["inflate"]["bad_reason"]) == (1, -(-len(raw) // 4096), im.CRC)
    assert bad["carried_bytes"] == st["carried_bytes"] and bad["header_done"] == 1
    b, _, nr2, st2 = ctx.bam_in_feed(im.bgzip(raw[8192:], 4096, eof=True), last=True)
    assert a + b == t1 and nr + nr2 == 20 * 64 and st2["carried_bytes"] == 0


def test_other_results_are_left_alone(rig, small_case):
    """a pointer bgzf_compress returned, a text bgzf_inflate returned, the resident batch and a pending screen_fetch survive a feed"""
    capi, idx, ctx = rig
    L = capi.lib()
    from tests import test_host_bgzf as hz
    sam = hz.golden("align_small.sam")
    buf = np.frombuffer(sam, dtype=np.uint8)
    p = capi.BgzfParamsC(65280, 1, 1, 0)
    out, n = C.c_void_p(), C.c_uint64()
    assert L.moni_bgzf_compress(ctx._h, buf.ctypes.data, buf.size, C.byref(p), C.byref(out), C.byref(n), None) == 0
    z = C.string_at(out.value, n.value)
    ip = capi.InflateParamsC()
    L.moni_inflate_params_default(C.byref(ip))
    zbuf = C.create_string_buffer(z, len(z))
    iout, inn = C.c_void_p(), C.c_uint64()
    assert L.moni_bgzf_inflate(ctx._h, zbuf, len(z), C.byref(ip), C.byref(iout), C.byref(inn), None) == 0
    synth = small_case.synth
    reads = synth.make_reads(small_case.pg, 300, 150, seed=5)
    offs = np.arange(0, (len(reads) + 1) * 150, 150, dtype=np.uint64)
    ctx.upload(reads.reshape(-1), offs)
    ctx.screen_run()
    raw, t1, _ = tiled(50)
    ctx.bam_in_reset()
    assert ctx.bam_in_feed(im.bgzip(raw, 65280, 1, eof=True), last=True)[0] == t1
    assert C.string_at(out.value, n.value) == z, "the writer's buffer was touched"
    assert C.string_at(iout.value, inn.value) == sam, "the inflater's text was touched"
    res = ctx.screen_fetch()
    assert len(res) == len(reads) and np.array_equal(res, ctx.screen_batch(reads.reshape(-1), offs))


def test_files_without_the_end_of_file_member(rig):
    """last = 1 behind members that carry text: a header alone, and records, with no empty member at the end"""
    ctx = rig[2]
    ctx.bam_in_reset()
    a, b, nr, st = ctx.bam_in_feed(im.bgzip(bc.HDR, eof=False), last=True)
    assert (a, b, nr, st["records"], st["carried_bytes"], st["header_done"], st["inflate"]["blocks"]) == (b"", b"", 0, 0, 0, 1, 1)
    raw, t1, t2 = tiled(2, True)
    ctx.bam_in_reset()
    a, b, nr, st = ctx.bam_in_feed(im.bgzip(raw, 4096, eof=False), True, last=True)
    assert (a, b, nr, st["carried_bytes"]) == (t1, t2, 64, 0) and st["inflate"]["blocks"] == -(-len(raw) // 4096)
    ctx.bam_in_reset()
    assert ctx.bam_in_feed(im.bgzip(bc.HDR, eof=False))[3]["header_done"] == 1
    assert ctx.bam_in_feed(b"", last=True)[2] == 0          # nothing left over: a good end


def test_reset_between_two_files(rig):
    ctx = rig[2]
    raw, t1, _ = tiled(3)
    z = im.bgzip(raw, 4096, eof=True)
    ctx.bam_in_reset()
    cut = len(im.bgzip(raw[:4096], 4096))
    a, _, _, st = ctx.bam_in_feed(z[:cut])
    assert st["carried_bytes"] > 0 and st["header_done"] == 1
    rc, _, _, _, st = ctx.bam_in_feed(z, last=True, rc_only=True)          # a second file behind half a first: its header stands inside a record
    m = bm.Stream()
    m.feed(raw[:4096])
    with pytest.raises(bm.Bad) as e:
        m.feed(raw, True)
    assert rc == EINVAL and (st["bad_records"], st["first_bad_record"], st["bad_record_reason"]) == (1, e.value.index, e.value.reason)
    ctx.bam_in_reset()
    b, _, nr, st = ctx.bam_in_feed(z, last=True)
    assert b == t1 and nr == 3 * 64 and st["records"] == nr and st["carried_bytes"] == 0


def test_arguments(rig):
    capi, idx, ctx = rig
    L = capi.lib()
    raw, t1, _ = tiled(1)
    z = im.bgzip(raw, 65280, eof=True)
    buf = C.create_string_buffer(z, len(z))
    p1, p2, n1, n2, nr, st = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_uint64(), capi.BamInStatsC()
    good = capi.BamInParamsC()
    L.moni_bamin_params_default(C.byref(good))
    assert (good.paired, good.check_crc, list(good.reserved)) == (0, 1, [0, 0])

    def call(h=ctx._h, data=buf, ln=len(z), p=C.byref(good), last=1, a=C.byref(p1), an=C.byref(n1), b=C.byref(p2), bn=C.byref(n2), r=C.byref(nr), s=C.byref(st)):
        return L.moni_bam_in_feed(h, data, ln, p, last, a, an, b, bn, r, s)

    ctx.bam_in_reset()
    assert call() == 0 and C.string_at(p1.value, n1.value) == t1 and n2.value == 0 and p2.value is None and nr.value == 64 and st.records == 64
    assert L.moni_bam_in_reset(None) == EINVAL
    for kw in (dict(h=None), dict(p=None), dict(a=None), dict(an=None), dict(b=None), dict(bn=None), dict(r=None), dict(data=None), dict(last=2), dict(last=-1)):
        assert call(**kw) == EINVAL, kw
    for field, k in (("paired", None), ("check_crc", None), ("reserved", 0), ("reserved", 1)):
        p = capi.BamInParamsC()
        L.moni_bamin_params_default(C.byref(p))
        if k is None:
            setattr(p, field, 2)
        else:
            p.reserved[k] = 1
        assert call(p=C.byref(p)) == EINVAL
    # len 0: nothing to do without last, nothing left over with it
    ctx.bam_in_reset()
    assert call(data=None, ln=0, last=0) == 0 and (n1.value, n2.value, nr.value, st.records, st.t_total >= 0) == (0, 0, 0, 0, True) and list(st.t_kernel) == [0, 0, 0, 0]
    assert call(data=None, ln=0, last=1) == 0 and n1.value == 0
    assert call(s=None) == 0 and n1.value == len(t1)
    ctx.bam_in_reset()
    with pytest.raises(RuntimeError, match="-22"):
        ctx.bam_in_feed(z[:-1])
