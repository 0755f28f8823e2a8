"""tests/bgzf_model.py against streams the test frames itself around zlib's raw DEFLATE output: what `walk` must take, and the damaged
copies it must refuse."""
import gzip
import os
import struct
import zlib

import pytest

from tests import bgzf_model as bm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def deflate1(data: bytes) -> bytes:
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def stream(data: bytes, block_size: int = bm.MAX_INPUT, eof: bool = True) -> bytes:
    out = b"".join(bm.frame(deflate1(data[at:at + block_size]), data[at:at + block_size]) for at in range(0, len(data), block_size))
    return out + (bm.EOF_BLOCK if eof else b"")


@pytest.fixture(scope="module")
def sam():
    return open(os.path.join(GOLDEN, "pe_small.sam"), "rb").read()


def test_walk_takes_zlib_streams(sam):
    for bs in (bm.MAX_INPUT, 4096):
        z = stream(sam, bs)
        blocks = bm.walk(z, bs)
        assert b"".join(b for b, _ in blocks) == sam and gzip.decompress(z) == sam
        assert len(blocks) == (len(sam) + bs - 1) // bs + 1 and blocks[-1] == (b"", 1)
        assert all(len(b) == bs for b, _ in blocks[:-2])
    assert bm.walk(b"") == [] and bm.walk(bm.EOF_BLOCK) == [(b"", 1)]
    stored = bm.frame(b"\x01\x03\x00\xfc\xffabc", b"abc")
    assert bm.walk(stored) == [(b"abc", 0)]


def test_walk_refuses_damage(sam):
    z = stream(sam[:5000], eof=False)
    assert len(bm.walk(z)) == 1
    n = len(z)
    bad_crc = z[:n - 8] + struct.pack("<I", struct.unpack_from("<I", z, n - 8)[0] ^ 1) + z[n - 4:]
    bad_isize = z[:n - 4] + struct.pack("<I", 4999)
    bad_bsize = z[:16] + struct.pack("<H", n) + z[18:]
    short_bsize = z[:16] + struct.pack("<H", n - 3) + z[18:]
    trailing = z + b"\x00"
    inner_trailing = bm.frame(deflate1(sam[:5000]) + b"\x00", sam[:5000])
    # one member, two DEFLATE blocks: the first without BFINAL
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    two = c.compress(sam[:2500]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(sam[2500:5000]) + c.flush()
    two_blocks = bm.frame(two, sam[:5000])
    assert gzip.decompress(two_blocks) == sam[:5000]          # a valid gzip member, and yet no BGZF block of ours
    bad_magic = b"\x1f\x8b\x08\x00" + z[4:]
    bad_subfield = z[:12] + b"BD" + z[14:]
    too_long = bm.frame(deflate1(sam[:bm.MAX_INPUT + 1]), sam[:bm.MAX_INPUT + 1])
    for what, s in (("crc", bad_crc), ("isize", bad_isize), ("bsize", bad_bsize), ("bsize short", short_bsize), ("trailing byte", trailing),
                    ("byte behind the deflate stream", inner_trailing), ("two-block member", two_blocks), ("flags", bad_magic),
                    ("subfield", bad_subfield), ("uncompressed size", too_long), ("cut", z[:-1])):
        with pytest.raises(bm.BgzfError):
            bm.walk(s)
            pytest.fail("walk took a stream with a wrong " + what)
    with pytest.raises(bm.BgzfError):
        bm.walk(stream(sam[:5000], eof=False), block_size=4096)


def test_order0_bytes():
    assert bm.order0_bytes(b"") == 0 and bm.order0_bytes(b"A" * 1000) == 0
    assert abs(bm.order0_bytes(b"ACGT" * 100) - 100.0) < 1e-9
    assert abs(bm.order0_bytes(bytes(range(256)) * 2, 256) - 512.0) < 1e-9
    # per block: two blocks of one letter each cost nothing, the same bytes in one block a bit each
    assert bm.order0_bytes(b"A" * 8 + b"C" * 8, 8) == 0 and abs(bm.order0_bytes(b"A" * 8 + b"C" * 8, 16) - 2.0) < 1e-9
    # the figures of DESIGN.md 7.11 for the golden files
    for name, want in (("align_small.sam", 11396), ("align_small_lifted.sam", 11023), ("pe_small.sam", 43150), ("pe_small_orphan.sam", 44567)):
        got = bm.order0_bytes(open(os.path.join(GOLDEN, name), "rb").read())
        assert abs(got - want) < 1.0, (name, got)
