"""tests/inflate_model.py held to the standard library: its inflater gives what zlib gives on every good input of tests/test_host_inflate.py, refuses
what zlib refuses, and its writer's blocks are DEFLATE to zlib."""
import gzip
import struct
import zlib

import pytest

from tests import inflate_model as im
from tests import test_host_inflate as hi


def members(z: bytes):
    at = 0
    while at < len(z):
        kind, total, po = im.member_at(z, at)
        yield z[at + po:at + total - 8], struct.unpack_from("<II", z, at + total - 8)
        at += total


@pytest.mark.parametrize("case", hi.GOOD, ids=[c[0] for c in hi.GOOD])
def test_model_equals_zlib(case):
    name, z, text = case
    m = hi.model(z)
    assert m["bad_blocks"] == 0 and m["text"] == text
    assert (gzip.decompress(z) if z else b"") == text
    parts = []
    for payload, (crc, isize) in members(z):
        d = zlib.decompressobj(-15)
        raw = d.decompress(payload)
        assert d.eof and not d.unused_data and len(raw) == isize and (zlib.crc32(raw) & 0xFFFFFFFF) == crc
        parts.append(raw)
    assert b"".join(parts) == text
    assert m["stored"] + m["fixed"] + m["dynamic"] == sum(len(t) for t in m["types"]) >= m["blocks"]


@pytest.mark.parametrize("case", hi.DAMAGED, ids=[c[0] for c in hi.DAMAGED])
def test_zlib_refuses_what_the_model_refuses(case):
    name, z, reason = case
    m = hi.model(z)
    assert (m["bad_blocks"], m["bad_reason"], m["text"]) == (1, reason, b"")
    with pytest.raises((zlib.error, gzip.BadGzipFile, EOFError, OSError)):
        gzip.decompress(z)
    if reason not in (im.HEADER, im.ISIZE, im.OVERRUN, im.CRC, im.TRAILING):          # the DEFLATE stream itself is bad
        payload, (crc, isize) = next(members(z))
        d = zlib.decompressobj(-15)
        try:
            d.decompress(payload)
            assert not d.eof
        except zlib.error:
            pass


def test_reasons_are_the_header_s():
    import re
    from moni_align_amd import capi
    import os
    h = open(os.path.join(os.path.dirname(capi.HERE), "include", "moni_hip.h")).read()
    names = re.findall(r"MONI_INF_([A-Z_]+)", h[h.index("enum { MONI_INF_OK"):h.index("MONI_INF_CRC };")] + "MONI_INF_CRC")
    assert tuple(names) == capi.INF_REASONS
    assert [getattr(im, n) for n in names] == list(range(12))


def test_bit_writer_round_trip():
    W = im.stored_block(b"abc", last=False)
    im.fixed_block([ord("x"), (5, 1), (258, 4)], W=W)
    text, types, reason = im.inflate_payload(W.bytes(), 3 + 6 + 258)
    assert reason == im.OK and types == [0, 1] and text == zlib.decompress(W.bytes(), -15)
    for n in range(3, 259):
        s, ev, eb = im.len_symbol(n)
        assert im.LEN_BASE[s - 257] + ev == n and ev < (1 << eb) or eb == 0 and ev == 0
    for d in (1, 2, 4, 5, 24576, 24577, 32768):
        s, ev, eb = im.dist_symbol(d)
        assert im.DIST_BASE[s] + ev == d and ev < (1 << eb) or eb == 0 and ev == 0
