"""BGZF as the SAM specification (4.1) and this project's DESIGN.md 7.11 fix it, in plain Python over the standard library: a strict reader
(`walk`) and the order-0 entropy bound of the compression condition (`order0_bytes`).  No project code."""
import math
import struct
import zlib

HEADER = bytes.fromhex("1f8b08040000000000ff0600424302 00".replace(" ", ""))          # the 16 bytes before BSIZE
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
MAX_BLOCK = 65536          # bytes of a BGZF block at most
MAX_INPUT = 65280          # uncompressed bytes of a block at most

assert len(HEADER) == 16 and len(EOF_BLOCK) == 28


class BgzfError(ValueError):
    pass


def frame(payload: bytes, data: bytes) -> bytes:
    """one BGZF block around a raw DEFLATE stream `payload` that inflates to `data`"""
    total = 18 + len(payload) + 8
    return HEADER + struct.pack("<H", total - 1) + payload + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data))


def walk(data: bytes, block_size: int = MAX_INPUT):
    """Parses `data` member by member; returns [(uncompressed bytes, BTYPE)] or raises BgzfError.  Every header byte is fixed: magic, CM 8,
    FLG 4, MTIME 0, XFL 0, OS 255, XLEN 6, the `BC` subfield of length 2, BSIZE = the member's length - 1.  The payload is exactly one DEFLATE
    block with BFINAL set, inflated with no dictionary and nothing left over; then CRC-32 and ISIZE of what came out."""
    out = []
    at = 0
    while at < len(data):
        if len(data) - at < 26:
            raise BgzfError("block at %d: %d bytes left, fewer than a header and a trailer" % (at, len(data) - at))
        if data[at:at + 16] != HEADER:
            raise BgzfError("block at %d: header bytes %s" % (at, data[at:at + 16].hex()))
        total = struct.unpack_from("<H", data, at + 16)[0] + 1
        if total < 26 + 1 or at + total > len(data) or total > MAX_BLOCK:
            raise BgzfError("block at %d: BSIZE + 1 = %d does not fit (%d bytes left)" % (at, total, len(data) - at))
        payload = data[at + 18:at + total - 8]
        first = payload[0]
        if not first & 1:
            raise BgzfError("block at %d: BFINAL is not set in the first DEFLATE block" % at)
        btype = (first >> 1) & 3
        if btype == 3:
            raise BgzfError("block at %d: BTYPE 11" % at)
        d = zlib.decompressobj(-15)
        try:
            raw = d.decompress(payload)
        except zlib.error as e:
            raise BgzfError("block at %d: %s" % (at, e))
        if not d.eof:
            raise BgzfError("block at %d: the DEFLATE stream does not end inside the payload" % at)
        if d.unused_data:
            raise BgzfError("block at %d: %d bytes behind the DEFLATE stream" % (at, len(d.unused_data)))
        crc, isize = struct.unpack_from("<II", data, at + total - 8)
        if isize != len(raw):
            raise BgzfError("block at %d: ISIZE %d, %d bytes inflated" % (at, isize, len(raw)))
        if crc != (zlib.crc32(raw) & 0xFFFFFFFF):
            raise BgzfError("block at %d: CRC-32 %08x, computed %08x" % (at, crc, zlib.crc32(raw) & 0xFFFFFFFF))
        if len(raw) > min(block_size, MAX_INPUT):
            raise BgzfError("block at %d: %d uncompressed bytes" % (at, len(raw)))
        out.append((raw, btype))
        at += total
    return out


def order0_bytes(data: bytes, block_size: int = MAX_INPUT) -> float:
    """the sum over the blocks of `data` of the order-0 entropy of the block's bytes, in bytes"""
    total = 0.0
    for at in range(0, len(data), block_size):
        blk = data[at:at + block_size]
        counts = [0] * 256
        for b in blk:
            counts[b] += 1
        total += -sum(c * math.log2(c / len(blk)) for c in counts if c) / 8.0
    return total
