"""infl_member (moni_align_amd/csrc/inflate_core.h: what inflate_member_kernel runs per BGZF member) replayed on the host, lanes as loops and
phases in launch order, against tests/inflate_model.py: the bytes, the DEFLATE blocks by BTYPE, and for damaged streams the lowest bad
member and its reason.  The real kernel is held to the same under -m gpu (tests/test_gpu_inflate.py)."""
import ctypes as C
import functools
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from moni_align_amd import capi
from tests import bgzf_model as bm
from tests import inflate_model as im
from tests import test_host_bgzf as hb

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sim")
EINVAL = -22
TWO_RECORDS = b"@a\nACGTACGT\n+\nIIIIIIII\n@b\nACGT\n+\nIIII\n"          # the file of tests/test_cli_bgzf.py
_lib = None


def sim_lib():
    """tests/host_sim/libinflate_sim.so, built beside the other replays and leaving them alone"""
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "libinflate_sim.so")
        src = os.path.join(HERE, "inflate_sim.cpp")
        deps = [src, os.path.join(capi.CSRC, "inflate_core.h"), os.path.join(capi.CSRC, "bgzf_core.h"), os.path.join(os.path.dirname(capi.HERE), "include", "moni_hip.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
        L = C.CDLL(so)
        L.inflsim_scan.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.inflsim_inflate.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
        _lib = L
    return _lib


STAT_KEYS = ("blocks", "bad_blocks", "first_bad_block", "bad_reason", "stored", "fixed", "dynamic")


def sim_scan(z: bytes):
    buf = np.frombuffer(z, dtype=np.uint8)
    n, used, ob = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = sim_lib().inflsim_scan(buf.ctypes.data if len(z) else None, len(z), C.byref(n), C.byref(used), C.byref(ob))
    return rc, n.value, used.value, ob.value


def sim_inflate(z: bytes, check_crc: bool = True):
    """the replay's (return code, text, stats: STAT_KEYS); the text buffer is exactly the sum of ISIZE"""
    buf = np.frombuffer(z, dtype=np.uint8)
    _, _, _, ob = sim_scan(z)
    out = np.zeros(ob, dtype=np.uint8)
    n, st = C.c_uint64(), np.zeros(7, dtype=np.uint64)
    rc = sim_lib().inflsim_inflate(buf.ctypes.data if len(z) else None, len(z), 1 if check_crc else 0, out.ctypes.data if ob else None, ob, C.byref(n), st.ctypes.data)
    return rc, out[:n.value].tobytes(), dict(zip(STAT_KEYS, (int(x) for x in st)))


@functools.lru_cache(maxsize=None)
def model(z: bytes, check_crc: bool = True):
    return im.inflate(z, check_crc)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fastq_text(n: int = 65280, seed: int = 7) -> bytes:
    """n bytes of FASTQ: 150 random bases and 150 qualities out of 41 letters per record"""
    rng = np.random.default_rng(seed)
    out, i = bytearray(), 0
    while len(out) < n:
        out += b"@read%d\n%s\n+\n%s\n" % (i, bytes(rng.choice(list(b"ACGT"), 150).tolist()), (rng.integers(0, 41, 150) + 33).astype(np.uint8).tobytes())
        i += 1
    return bytes(out[:n])


def random_bytes(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def far_repeat() -> bytes:
    """300 random bytes, 31700 letters of ACGT, the 300 again: matches at distance 32000, the farthest zlib looks being 32768 - 262"""
    a = random_bytes(300, 11)
    return a + bytes(np.random.default_rng(12).choice(list(b"ACGT"), 31700).tolist()) + a


def member(payload, text: bytes, extra: bytes = b"") -> bytes:
    return im.frame(payload.bytes() if isinstance(payload, im.BitWriter) else payload, text, extra)


def lens(d) -> list:
    """{symbol: length} as the list of literal/length lengths up to the last symbol that has one"""
    out = [0] * max(257, max(d) + 1)
    for k, v in d.items():
        out[k] = v
    return out


def lengths_1_to_15():
    """A literal/length code with one code of every length 1..14 and two of 15 (Kraft sum 1): twelve literals on the short codes, the lengths
    3, 11..12 and 258 and the end of the block on the codes of 13, 14, 15 and 15 bits, behind the first-level table.  Distances: 1 2 3 4 5 5 bits."""
    lits = b"ACGTN\n@+IF#:"
    ll = [0] * 286
    for k, b in enumerate(lits):
        ll[b] = k + 1
    ll[257], ll[265], ll[285], ll[256] = 13, 14, 15, 15
    dl = [1, 2, 3, 4, 5, 5]
    tokens = list(lits) + [(3, 1), (12, 5), (11, 8), (258, 2), ord("A"), (258, 7), (3, 3)]
    text = bytearray(lits)
    for t in tokens[len(lits):]:
        if isinstance(t, int):
            text.append(t)
        else:
            for _ in range(t[0]):
                text.append(text[-t[1]])
    return member(im.dynamic_block(tokens, ll, dl), bytes(text)), bytes(text)


def repeat_across_boundary():
    """257 literal/length and 8 distance lengths whose last run of 3s is sent as 3, 16 x 6, 16 x 5: the first repeat covers the lengths of the symbols
    254 255 256 and of the distances 0 1 2"""
    ll = [0] * 257
    ll[65] = ll[66] = 2
    ll[253] = ll[254] = ll[255] = ll[256] = 3
    dl = [3] * 8
    syms = [(18, 65), 2, 2, (18, 138), (18, 48), 3, (16, 6), (16, 5)]
    text = bytes([65, 66, 253, 254, 255, 65, 65])
    return member(im.dynamic_block(list(text), ll, dl, cl_syms=syms), text), text


@functools.lru_cache(maxsize=None)
def good_cases():
    """(name, stream, text): the inputs of the issue; tests/test_gpu_inflate.py sends the same ones through the kernel"""
    fq = fastq_text()
    c = [("empty", b"", b""), ("eof_alone", bm.EOF_BLOCK, b""), ("eof_after_data", im.bgzip(TWO_RECORDS, eof=True), TWO_RECORDS),
         ("len1", im.bgzip(b"A"), b"A"), ("len2", im.bgzip(b"AC"), b"AC"), ("acgt4", im.bgzip(b"ACGT" * 4), b"ACGT" * 4), ("runs", im.bgzip(b"A" * 1000), b"A" * 1000),
         ("two_records", im.bgzip(TWO_RECORDS), TWO_RECORDS)]
    c += [("fastq/level%d" % lv, im.bgzip(fq, level=lv), fq) for lv in (1, 6, 9, 0)]
    c += [("fastq/fixed", im.bgzip(fq, strategy=zlib.Z_FIXED), fq), ("random65280", im.bgzip(random_bytes(65280, 3)), random_bytes(65280, 3)),
          ("far_repeat", im.bgzip(far_repeat(), level=9), far_repeat())]
    big = (fq + fq)[:65536]
    c += [("isize65536", bm.frame(im.deflate_raw(big), big), big)]
    c += [("lengths_1_to_15",) + lengths_1_to_15(), ("one_distance_code", member(im.dynamic_block([65, (10, 1)], lens({65: 1, 256: 2, 264: 2}), [1]), b"A" * 11), b"A" * 11)]
    ll = lens({65: 1, 67: 2, 256: 2})
    c += [("no_distance_code", member(im.dynamic_block([65, 67, 65], ll, [0]), b"ACA"), b"ACA"),
          ("only_end_of_block", member(im.dynamic_block([], [0] * 256 + [1], [0]), b""), b""),
          ("repeat_across_boundary",) + repeat_across_boundary()]
    for name in hb.SAMS:
        sam = hb.golden(name)
        c += [("own_writer/" + name, hb.sim_compress(sam, 65280, 1, True)[0], sam)]
    small = fastq_text(3000, 5)
    c += [("bs1", im.bgzip(small[:400], 1), small[:400]), ("bs37", im.bgzip(small, 37), small), ("bs4096", im.bgzip(hb.golden("pe_small.sam"), 4096), hb.golden("pe_small.sam")),
          ("bs65280", im.bgzip(hb.golden("pe_small.sam"), 65280, eof=True), hb.golden("pe_small.sam"))]
    many = fastq_text(100000, 9)
    c += [("members2500", im.bgzip(many, 40), many)]
    # a stored block, a fixed block that reaches into it, a dynamic block that reaches into both, in one member
    W = im.stored_block(b"ACGTACGTTT", last=False)
    im.fixed_block([(8, 10), ord("N")], last=False, W=W)
    im.dynamic_block([(5, 19), 65, (4, 1)], lens({65: 1, 256: 2, 258: 3, 259: 3}), [1, 0, 0, 0, 0, 0, 0, 0, 1], W=W)
    text = b"ACGTACGTTT" + b"ACGTACGT" + b"N" + b"ACGTA" + b"A" + b"AAAA"
    c += [("three_kinds", member(W, text), text)]
    # the farthest match there is: 32768 back, out of a stored block
    far = random_bytes(32768, 13)
    c += [("distance32768", member(im.fixed_block([(258, 32768), (42, 32768)], W=im.stored_block(far, last=False)), far + far[:300]), far + far[:300])]
    return tuple(c)


def patch(z: bytes, at: int, value: int) -> bytes:
    return z[:at] + bytes([value]) + z[at + 1:]


def reframe(z: bytes, payload=None, isize=None, crc=None) -> bytes:
    """the single member z with another payload, ISIZE or CRC-32 (BSIZE follows the payload)"""
    total = struct.unpack_from("<H", z, 16)[0] + 1
    pl = z[18:total - 8] if payload is None else payload
    c, n = struct.unpack_from("<II", z, total - 8)
    return z[:16] + struct.pack("<H", 18 + len(pl) + 8 - 1) + pl + struct.pack("<II", c if crc is None else crc, n if isize is None else isize)


@functools.lru_cache(maxsize=None)
def damaged_cases():
    """(name, stream, the one reason it trips)"""
    good = im.bgzip(fastq_text(3000, 5))
    text = fastq_text(3000, 5)
    ll = [0] * 257
    ll[65], ll[67], ll[256] = 1, 2, 2
    over = list(ll)
    over[66] = 1          # 1/2 + 1/2 + 1/4 + 1/4
    crc = struct.unpack_from("<I", good, len(good) - 8)[0]
    stored = member(im.stored_block(b"ACGT"), b"ACGT")
    c = [("header_byte", patch(good, 2, 9), im.HEADER),
         ("btype3", member(bytes([7]), b""), im.BTYPE),
         ("stored_len", member(im.stored_block(b"ACGT", nlen=0x1234), b"ACGT"), im.STORED_LEN),
         ("over_subscribed", member(im.dynamic_block([65], over, [0]), b"A"), im.CODE_LENGTHS),
         ("repeat_without_previous", member(im.dynamic_block([65], ll, [0], cl_syms=[(16, 3)] + ll[3:] + [0]), b"A"), im.CODE_LENGTHS),
         ("literal_286", member(im.fixed_block([65, ("sym", 286)]), b"A"), im.BAD_SYMBOL),
         ("distance_30", member(im.fixed_block([65, 65, 65, ("dsym", 3, 30)]), b"AAA"), im.BAD_SYMBOL),
         ("distance_before_start", member(im.fixed_block([65, 67, (3, 3)]), b"AC"), im.DISTANCE),
         ("isize_small", reframe(good, isize=2999), im.OVERRUN),
         ("isize_large", reframe(good, isize=3001), im.ISIZE),
         ("payload_cut", reframe(good, payload=good[18:len(good) - 8 - 5]), im.TRUNCATED),
         ("stored_cut", reframe(stored, payload=stored[18:len(stored) - 8 - 2]), im.TRUNCATED),
         ("spare_byte", reframe(good, payload=good[18:len(good) - 8] + b"\0"), im.TRAILING),
         ("crc_bit", reframe(good, crc=crc ^ 0x10000), im.CRC)]
    return tuple(c), text


# ---- the replay against the model ---------------------------------------------------------------------------------------------------------
GOOD = good_cases()
DAMAGED, DAMAGED_TEXT = damaged_cases()


@pytest.mark.parametrize("case", GOOD, ids=[c[0] for c in GOOD])
def test_good_stream(case):
    name, z, text = case
    m = model(z)
    assert m["bad_blocks"] == 0 and m["text"] == text, "the case itself is wrong"
    rc, got, st = sim_inflate(z)
    assert rc == 0 and got == text
    assert st == {k: m[k] for k in STAT_KEYS}
    assert sim_scan(z) == (0, m["blocks"], len(z), len(text))


def test_cases_are_what_they_claim():
    m = {c[0]: model(c[1]) for c in GOOD}
    assert m["acgt4"]["types"] == [[1]] and m["eof_alone"]["types"] == [[1]] and m["eof_after_data"]["blocks"] == 2
    assert m["fastq/level0"]["types"] == [[0, 0]] and set(m["fastq/fixed"]["types"][0]) == {1} and m["random65280"]["types"][0] == [0] * len(m["random65280"]["types"][0])
    assert len(m["random65280"]["types"][0]) > 2
    assert m["members2500"]["blocks"] == 2500 and m["bs1"]["blocks"] == 400
    assert m["three_kinds"]["types"] == [[0, 1, 2]] and m["distance32768"]["types"] == [[0, 1]]
    for name, z, text in GOOD:
        if name in ("fastq/level1", "fastq/level6", "fastq/level9", "far_repeat", "runs", "acgt4", "isize65536"):
            tr = []
            total = struct.unpack_from("<H", z, 16)[0] + 1
            assert im.inflate_payload(z[18:total - 8], len(text), tr)[2] == im.OK
            if name.startswith("fastq/level"):
                assert len(tr) > 1 and any(b[1] < b[0] for b in tr[1:]), "no later block reaches back past its own start: the case proves nothing"
            if name == "far_repeat":
                assert max(b[2] for b in tr) == 32000          # distance code 29
            if name == "runs":
                assert max(b[2] for b in tr) == 1
            if name == "acgt4":
                assert tr[0][2] == 4
            if name == "isize65536":
                assert len(text) == 65536
    # our own writer's streams hold the two RFC 1951 allowances: a block without a distance code, and one with a single one
    assert all(t == 2 or t == 0 for c in GOOD if c[0].startswith("own_writer/") for tt in model(c[1])["types"][:-1] for t in tt)


@pytest.mark.parametrize("case", DAMAGED, ids=[c[0] for c in DAMAGED])
def test_damaged_stream(case):
    name, z, reason = case
    m = model(z)
    assert (m["bad_blocks"], m["first_bad_block"], m["bad_reason"]) == (1, 0, reason), "the case itself is wrong"
    rc, got, st = sim_inflate(z)
    assert rc == EINVAL and got == b""
    assert st == {k: m[k] for k in STAT_KEYS}
    with pytest.raises(Exception):
        gzip.decompress(z)


def test_crc_is_not_looked_at_when_told_so():
    z = dict((c[0], c[1]) for c in DAMAGED)["crc_bit"]
    rc, got, st = sim_inflate(z, check_crc=False)
    assert rc == 0 and got == DAMAGED_TEXT and st["bad_blocks"] == 0
    assert model(z, False)["text"] == DAMAGED_TEXT


def test_lowest_bad_member_is_reported():
    good = im.bgzip(fastq_text(3000, 5), 500)
    bad = dict((c[0], c[1]) for c in DAMAGED)
    z = good + bad["distance_before_start"] + good + bad["crc_bit"] + good
    m = model(z)
    assert (m["bad_blocks"], m["first_bad_block"], m["bad_reason"]) == (2, 6, im.DISTANCE)
    rc, got, st = sim_inflate(z)
    assert rc == EINVAL and got == b"" and st == {k: m[k] for k in STAT_KEYS}
    # a member that is no BGZF behind a bad one: the bad one is the lowest
    z = good + bad["crc_bit"] + good + b"\x1f\x8b\x08\x00" + bytes(30)
    m = model(z)
    assert (m["first_bad_block"], m["bad_reason"], m["bad_blocks"]) == (6, im.CRC, 2)
    assert sim_inflate(z)[2] == {k: m[k] for k in STAT_KEYS}


def test_scan():
    text = fastq_text(3000, 5)
    z = im.bgzip(text, 500, eof=True)
    sizes = [struct.unpack_from("<H", z, 16)[0] + 1]
    # cut in the middle of the third member: two members, their bytes, their text
    at = 0
    for _ in range(2):
        at += struct.unpack_from("<H", z, at + 16)[0] + 1
    for cut in (at, at + 1, at + 11, at + 12, at + 17, at + 30):
        assert sim_scan(z[:cut]) == (0, 2, at, 1000) and im.scan(z[:cut]) == (True, 2, at, 1000)
    assert sim_scan(z) == (0, 7, len(z), 3000) and sizes[0] > 26
    # `BC` behind another subfield
    other = member(im.deflate_raw(text[:500]), text[:500], extra=b"XY\x03\0abc")
    assert sim_scan(other + z) == (0, 8, len(other) + len(z), 3500)
    rc, got, st = sim_inflate(other + z)
    assert rc == 0 and got == text[:500] + text and model(other + z)["text"] == got
    # plain gzip is not BGZF; neither is a member whose BSIZE leaves no room for the trailer
    assert sim_scan(gzip.compress(text))[0] == EINVAL and im.scan(gzip.compress(text))[0] is False
    assert sim_scan(z[:at] + gzip.compress(text))[:3] == (EINVAL, 2, at)
    assert sim_scan(patch(z, 16, 20))[0] == EINVAL
    # inflate wants whole members
    rc, got, st = sim_inflate(z[:at + 30])
    assert rc == EINVAL and (st["bad_blocks"], st["first_bad_block"], st["bad_reason"]) == (1, 2, im.TRUNCATED)
    assert st == {k: model(z[:at + 30])[k] for k in STAT_KEYS}


def test_library_scan_needs_no_gpu():
    """moni_bgzf_scan of the library itself (host only)"""
    import __graft_entry__
    __graft_entry__.build()
    z = im.bgzip(fastq_text(3000, 5), 500, eof=True)
    assert capi.bgzf_scan(z) == (0, 7, len(z), 3000)
    assert capi.bgzf_scan(z[:-1]) == (0, 6, len(z) - 28, 3000)
    assert capi.bgzf_scan(gzip.compress(b"ACGT"))[0] == EINVAL
    assert capi.bgzf_scan(b"") == (0, 0, 0, 0)
