"""The inputs of the BAM reader's tests (tests/test_host_bamin.py on the replay, tests/test_gpu_bamin.py on the kernels): uncompressed BAM
streams made by bamin_model's writer, with how each is cut into BGZF members and fed.  A case is (name, raw, paired, member, per_call): the
stream goes into members of `member` bytes of text, `per_call` of them a call (0: all in one), the last call with `last` set.  Sizes that depend
on the segment are derived from S, which the replay reports."""
import functools
import struct

import numpy as np

from tests import bamin_model as bm

HDR = bm.header()
REFS3000 = bm.header(b"@HD\tVN:1.6\n", [(b"contig%04d" % i, 1000 + i) for i in range(3000)])


def read(i, n, seed=0, flag=4, name=None, **kw):
    rng = np.random.default_rng(1000 * seed + i)
    seq = bytes(rng.choice(list(b"ACGT"), n).tolist())
    return bm.record(name if name is not None else b"r%d" % i, seq, rng.integers(0, 41, n).astype(np.uint8).tobytes(), flag, **kw)


def pair(i, n1, n2, seed=0, f1=0x4D, f2=0x8D, name=None):
    nm = name if name is not None else b"p%d" % i
    return read(2 * i, n1, seed, f1, nm) + read(2 * i + 1, n2, seed, f2, nm)


def pad_to(prefix_len: int, target: int, i: int = 0) -> bytes:
    """a record that ends at `target` behind a prefix of prefix_len bytes: ten bases and a B tag of filler"""
    base = read(i, 10, 99, name=b"pad%d" % i, tags=b"")
    fill = target - prefix_len - len(base) - 8
    assert fill >= 0
    r = read(i, 10, 99, name=b"pad%d" % i, tags=b"XBBC" + struct.pack("<I", fill) + bytes(fill))
    assert prefix_len + len(r) == target
    return r


def decoy_words(n_bytes: int) -> bytes:
    """words that read as block_size 32 (every 4 bytes: a chain of period 36 from every one of them) with 300 and 68 mixed in"""
    w = [struct.pack("<I", 32)] * (n_bytes // 4)
    for k in range(5, len(w), 11):
        w[k] = struct.pack("<I", 300 if k & 1 else 68)
    return b"".join(w)


def cases(S: int):
    out = []

    def add(name, raw, paired=False, member=65280, per_call=0):
        out.append((name, raw, paired, member, per_call))

    add("header_only", HDR)
    add("header_3000_refs", REFS3000 + read(0, 50), member=4096, per_call=1)
    add("one_record", HDR + read(0, 100))
    for n in (1, 2, 7, 0):
        add("l_seq_%d" % n, HDR + read(0, n) + read(1, 33))
    add("short_name_tags_cigar", HDR + read(0, 21, name=b"x", flag=0, cigar=(20 << 4, 1 << 4 | 4), tags=b"NMC\x02RGZgrp1\x00", ref=0, pos=7))
    add("no_qualities", HDR + bm.record(b"nq", b"ACGTN", None) + bm.record(b"nq_rev", b"AACGT", None, 0x10))
    nib = bytes(range(16))
    packed = bytes(nib[i] << 4 | nib[i + 1] for i in range(0, 16, 2))
    add("every_nibble", HDR + bm.record(b"fwd", b"", bytes(range(16)), 0, nibbles=(16, packed)) + bm.record(b"rev", b"", bytes(range(16)), 0x10, nibbles=(16, packed)) +
        bm.record(b"rev_odd", b"", bytes(range(15)), 0x10, nibbles=(15, packed)))
    mixed = HDR + read(0, 40) + read(1, 40, flag=0x100) + read(2, 40, flag=0x800) + read(3, 0) + read(4, 41) + read(5, 30, flag=0x904)
    add("secondary_between", mixed)
    prs = HDR + pair(0, 50, 51) + read(90, 30, flag=0x141, name=b"p1") + read(2, 50, 0, 0x4D, b"p1") + read(91, 30, flag=0x800 | 0x4D, name=b"p1") + read(92, 0, flag=0x4D, name=b"p1") + \
        read(3, 52, 0, 0x8D, b"p1") + read(93, 20, flag=0x100) + pair(2, 10, 11)
    add("secondary_inside_pairs", prs, paired=True)
    # positions against a segment's edge
    first = pad_to(len(HDR), S)
    add("starts_at_S", HDR + first + read(1, 60) + read(2, 61))
    add("ends_at_S", HDR + first)
    for k in (1, 2, 3):
        add("block_size_across_S_%d" % k, HDR + pad_to(len(HDR), S - k) + read(1, 60) + read(2, 61))
    add("longer_than_S", HDR + read(0, 30) + read(1, 70000, flag=0x10) + read(2, 31))
    add("longer_than_2S", HDR + read(0, 30) + read(1, 200000) + read(2, 31) + read(3, 32, flag=0x10))
    # wrong candidates in long chains across the edges: a B tag of 2.5 segments, qualities of 32 0 0 0, a name with the same
    dec = HDR + read(0, 30) + read(1, 20, tags=b"XDBI" + struct.pack("<I", 5 * S // 8) + decoy_words(5 * S // 2)) + \
        bm.record(b"q" + decoy_words(200)[1:], b"ACGT" * 300, decoy_words(1200)) + read(2, 45) + \
        read(3, 20, tags=b"XDBI" + struct.pack("<I", S // 4 + 1) + b"\x00" + decoy_words(S)) + read(4, 46)
    add("decoys", dec)
    add("decoys_cut", dec, member=4096, per_call=3)
    # members and calls
    small = HDR + b"".join(read(i, 20 + i % 9, 3, flag=(0x10 if i % 3 == 0 else 4)) for i in range(40))
    many = HDR + b"".join(read(i, 100 + i % 50, 4) for i in range(600))
    spairs = HDR + b"".join(pair(i, 20 + i % 7, 25 - i % 5, 5) for i in range(20))
    mpairs = HDR + b"".join(pair(i, 100 + i % 7, 95 - i % 5, 6) for i in range(300))
    for member, raw, praw in ((37, small, spairs), (100, small, spairs), (4096, many, mpairs), (65280, many + many[len(HDR):], mpairs + mpairs[len(HDR):])):
        for per_call in (1, 3, 0):
            add("members_%d_by_%d" % (member, per_call), raw, False, member, per_call)
            add("pairs_%d_by_%d" % (member, per_call), praw, True, member, per_call)
    # the last record ends 1 to 3 bytes before the call's end: the bytes behind it are the start of the next block_size
    two = read(0, 33) + read(1, 34)
    for k in (1, 2, 3):
        add("carry_of_%d" % k, HDR + two + read(2, 35), member=len(HDR) + len(two) + k, per_call=1)
    return out


def bad_cases(S: int):
    """(name, raw, paired, member, per_call, index, reason)"""
    out = []
    good = b"".join(read(i, 40) for i in range(6))
    r2 = read(2, 40)

    def with_size(r, bs):
        return struct.pack("<I", bs) + r[4:]

    def patched(r, at, b):
        return r[:at] + bytes([b]) + r[at + 1:]

    out.append(("magic", b"BAM\x02" + HDR[4:] + good, False, 65280, 0, 0, bm.MAGIC))
    out.append(("magic_short", b"BA", False, 65280, 0, 0, bm.TRUNCATED))
    out.append(("magic_short_wrong", b"BX", False, 65280, 0, 0, bm.MAGIC))
    out.append(("l_text_negative", b"BAM\x01" + struct.pack("<i", -1) + bytes(8), False, 65280, 0, 0, bm.HEADER))
    out.append(("ref_name_0", bm.header(b"", [(b"a", 5)])[:12] + struct.pack("<i", 0) + bytes(8), False, 65280, 0, 0, bm.HEADER))
    three = read(0, 40) + read(1, 40)
    out.append(("block_size_31", HDR + three + with_size(r2, 31) + good, False, 65280, 0, 2, bm.BLOCK_SIZE))
    out.append(("block_size_2^28+1", HDR + three + with_size(r2, (1 << 28) + 1) + good, False, 65280, 0, 2, bm.BLOCK_SIZE))
    out.append(("l_read_name_0", HDR + three + patched(r2, 12, 0) + good, False, 65280, 0, 2, bm.FIELDS))
    out.append(("name_without_nul", HDR + three + patched(r2, 36 + 2, ord("x")) + good, False, 65280, 0, 2, bm.FIELDS))
    out.append(("fields_beyond_block", HDR + three + r2[:20] + struct.pack("<i", 4000) + r2[24:] + good, False, 65280, 0, 2, bm.FIELDS))
    out.append(("l_seq_negative", HDR + three + r2[:20] + struct.pack("<i", -5) + r2[24:] + good, False, 65280, 0, 2, bm.FIELDS))
    out.append(("bad_among_good_lowest", HDR + three + patched(r2, 12, 0) + good + with_size(r2, 5) + good, False, 65280, 0, 2, bm.FIELDS))
    out.append(("bad_in_second_call", HDR + good + patched(r2, 12, 0) + good, False, len(HDR) + len(good) // 2, 1, 6, bm.FIELDS))
    out.append(("bad_behind_the_edge", HDR + pad_to(len(HDR), S - 2) + three + with_size(r2, 7) + good, False, 65280, 0, 3, bm.BLOCK_SIZE))
    out.append(("cut_record", HDR + good[:-5], False, 65280, 0, 5, bm.TRUNCATED))
    out.append(("cut_header", REFS3000[:-3], False, 4096, 1, 0, bm.TRUNCATED))
    p = pair(0, 30, 31) + pair(1, 32, 33)
    out.append(("lone_first_mate", HDR + p + read(8, 30, 0, 0x4D, b"p4"), True, 65280, 0, 4, bm.TRUNCATED))
    out.append(("names_differ", HDR + p + read(8, 30, 0, 0x4D, b"p4") + read(9, 30, 0, 0x8D, b"p5") + p, True, 65280, 0, 5, bm.PAIRING))
    out.append(("first_twice", HDR + p + read(8, 30, 0, 0x4D, b"p4") + read(9, 30, 0, 0x4D, b"p4") + p, True, 65280, 0, 5, bm.PAIRING))
    out.append(("second_first", HDR + read(8, 30, 0, 0x8D, b"p4") + read(9, 30, 0, 0x4D, b"p4") + p, True, 65280, 0, 0, bm.PAIRING))
    out.append(("not_paired_flag", HDR + p + read(8, 30, 0, 4, b"p4") + read(9, 30, 0, 0x8D, b"p4") + p, True, 65280, 0, 4, bm.PAIRING))
    out.append(("pairing_before_fields", HDR + p + read(8, 30, 0, 0x8D, b"p4") + patched(r2, 12, 0) + p, True, 65280, 0, 4, bm.PAIRING))
    out.append(("sorted_pairs", HDR + read(0, 30, 0, 0x41, b"a") + read(1, 30, 0, 0x41, b"b") + read(2, 30, 0, 0x81, b"a") + read(3, 30, 0, 0x81, b"b"), True, 65280, 0, 1, bm.PAIRING))
    return out


def chunks(raw: bytes, member: int, per_call: int):
    """the inflated bytes of each call"""
    step = member * per_call if per_call else max(len(raw), 1)
    return [raw[at:at + step] for at in range(0, max(len(raw), 1), step)]


@functools.lru_cache(maxsize=None)
def model_run(raw: bytes, paired: bool, member: int, per_call: int):
    """('ok', text1, text2, [the counts of each call]) or ('bad', index, reason, the call that failed)"""
    st, t1, t2, calls = bm.Stream(paired), [], [], []
    parts = chunks(raw, member, per_call)
    for k, part in enumerate(parts):
        try:
            r = st.feed(part, k + 1 == len(parts))
        except bm.Bad as e:
            return ("bad", e.index, e.reason, k)
        t1.append(r.pop("text1"))
        t2.append(r.pop("text2"))
        calls.append(r)
    return ("ok", b"".join(t1), b"".join(t2), calls)
