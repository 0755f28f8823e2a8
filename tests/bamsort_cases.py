"""Inputs of the sorted-BAM tests (tests/test_host_bamsort.py on the CPU, tests/test_gpu_bamsort.py on the GPU): raw BAM records built field by
field, the issue's case list, the bad-record classes, and a BAM file assembled from tests/bgzf_model's framing.  TEST HARNESS."""
import struct
import zlib

import numpy as np

from tests import bam_model as bam
from tests import bamsort_model as bsm
from tests import bgzf_model as bgzf
from tests.test_bam_model import SAMS, golden

H1 = b"@HD\tVN:1.6\tSO:unknown\n@SQ\tSN:chr1\tLN:2147483647\n"
H2 = b"@HD\tVN:1.6\tSO:unknown\n@SQ\tSN:chr1\tLN:2147483647\n@SQ\tSN:chr2\tLN:600000000\n"
H300 = b"@HD\tVN:1.6\tSO:unknown\n" + b"".join(b"@SQ\tSN:c%d\tLN:%d\n" % (i, 100000 + i) for i in range(300))
SIZES = (40, 63, 64, 65, 127, 129, 1140)          # 1140: a read of 2000 bases takes more than 1100 bytes


def record(ref=0, pos=0, flag=0, ops=(), size=None, name=b"r", l_seq=None, seed=0) -> bytes:
    """one raw record; ops: [(length, letter)].  With `size` the record has exactly that many bytes (the name, SEQ/QUAL and filler share them)."""
    cigar = b"".join(struct.pack("<I", n << 4 | bam.OPS.index(c)) for n, c in ops)
    reflen = sum(n for n, c in ops if c in "MDN=X")
    if size is not None:
        rest = size - 36 - len(cigar)
        assert rest >= 2, "a record of %d bytes has no room for %d ops" % (size, len(ops))
        name = name[:rest - 1]
        rest -= len(name) + 1
        l_seq = (2 * rest) // 3 if l_seq is None else l_seq
        assert (l_seq + 1) // 2 + l_seq <= rest
    elif l_seq is None:
        l_seq = 0
    rng = np.random.default_rng(seed)
    body = bytes(rng.integers(0, 256, size=(l_seq + 1) // 2 + l_seq, dtype=np.uint8))
    fill = b"" if size is None else bytes(rng.integers(1, 256, size=size - 36 - len(cigar) - len(name) - 1 - len(body), dtype=np.uint8))
    fixed = struct.pack("<iiBBHHHiiii", ref, pos, len(name) + 1, 30, bam.reg2bin(pos, pos + max(reflen, 1)) & 0xFFFF, len(ops), flag, l_seq, -1, -1, 0)
    rec = fixed + name + b"\x00" + cigar + body + fill
    return struct.pack("<i", len(rec)) + rec


def offsets(recs) -> np.ndarray:
    return np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)


def _counts(n):
    return [record(ref=i % 3 - 1, pos=(i * 7919) % 1000 - 1 if i % 3 else -1, flag=16 if i & 1 else 0, ops=[(5, "M")] if SIZES[i % 7] >= 48 else (),
                   size=SIZES[i % 7], seed=i) for i in range(n)]


def _random(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        placed = rng.random() < 0.85
        ops = [(int(rng.integers(1, 200)), "MIDNSHP=X"[int(rng.integers(0, 9))]) for _ in range(int(rng.integers(0, 6)))] if placed else []
        out.append(record(ref=int(rng.integers(0, 2)) if placed else -1, pos=int(rng.integers(-1, 3000)) if placed else -1,
                          flag=int(rng.integers(0, 65536)), ops=ops, size=int(rng.integers(36 + 4 * len(ops) + 4, 700)), seed=seed + i))
    return out


def cases():
    """(name, header, [records]) - the issue's list"""
    c = [("n%d" % n, H2, _counts(n)) for n in (0, 1, 2, 63, 64, 65, 257)]
    c.append(("all_keys_equal", H1, [record(pos=5, size=40 + i, seed=i) for i in range(70)]))
    c.append(("both_strands", H1, [record(pos=5, flag=16 if i % 3 else 0, ops=[(3, "M")], size=60 + i, seed=i) for i in range(70)]))
    c.append(("pos_edges", H1, [record(pos=(-1, 2 ** 31 - 2, 0, 16383, -1, 7)[i % 6], ops=[(1, "M")], size=360 + i % 16, seed=i) for i in range(66)]))
    c.append(("unplaced_between", H2, [record(ref=-1 if i % 4 == 1 else i % 2, pos=-1 if i % 4 == 1 else 1000 - i, size=300 + i, seed=i) for i in range(80)]))
    c.append(("refs_300", H300, [record(ref=(i * 131) % 300, pos=i % 5, ops=[(2, "M")], size=50 + i % 40, seed=i) for i in range(600)]))
    c.append(("sorted", H1, [record(pos=i, size=48 + i % 9, seed=i) for i in range(130)]))
    c.append(("reversed", H1, [record(pos=129 - i, size=48 + i % 9, seed=i) for i in range(130)]))
    cig = [(), [(7, "M")], [(1, "M"), (1, "I")] * 35, [(4, "S"), (3, "M"), (2, "D"), (5, "N"), (1, "I"), (2, "="), (3, "X"), (9, "H"), (1, "P")], [(5, "S"), (6, "I")]]
    c.append(("cigars", H1, [record(pos=300 - 7 * i, ops=cig[i % 5], size=400 + i, seed=i) for i in range(40)]))
    for name in SAMS:
        h, lines = golden(name)
        c.append((name, h, bsm.split_records(bam.encode_records(h, lines))))
    c.append(("random2000", H2, _random(2000, 23)))
    return c


GOOD = [record(pos=i, ops=[(4, "M")], size=48, seed=i) for i in range(9)]


def _patch(rec: bytes, at: int, fmt: str, v) -> bytes:
    return rec[:at] + struct.pack("<" + fmt, v) + rec[at + struct.calcsize("<" + fmt):]


# (name, the bad record, its reason); OFFSET is made from the offsets (bad_batch)
BAD = [
    ("offset", None, "OFFSET"),
    ("short_ops", _patch(GOOD[0], 16, "H", 9), "SHORT"),
    ("short_name", _patch(GOOD[0], 12, "B", 200), "SHORT"),
    ("block_size", _patch(GOOD[0], 0, "i", 45), "SIZE"),
    ("name_0", _patch(GOOD[0], 12, "B", 0), "NAME"),
    ("ref_n_ref", _patch(GOOD[0], 4, "i", 1), "REF"),
    ("ref_minus_2", _patch(GOOD[0], 4, "i", -2), "REF"),
    ("pos_minus_2", _patch(GOOD[0], 8, "i", -2), "POS"),
    ("pos_2_31_minus_1", _patch(GOOD[0], 8, "i", 2 ** 31 - 1), "POS"),
]
REASONS = ("OK", "OFFSET", "SHORT", "SIZE", "NAME", "REF", "POS", "LENGTH")


def bad_batch(bad, at=5, second=None, second_at=7):
    """(records, offsets) with the bad record as record `at` among good ones (H1); for OFFSET the record's end is its start"""
    recs = list(GOOD)
    marks = []
    for b, where in ((bad, at),) + (((second, second_at),) if second is not None else ()):
        recs.insert(where, GOOD[0] if b[1] is None else b[1])
        if b[1] is None:
            marks.append(where)
    off = offsets(recs)
    for m in marks:
        off[m + 1] = off[m]          # the record behind it then has a size that is not its block_size's: a later bad record
    return b"".join(recs), off


def deflate_blocks(data: bytes, block_size: int, level: int = 1) -> bytes:
    """`data` as BGZF blocks of block_size bytes, one DEFLATE block each"""
    out = []
    for at in range(0, len(data), block_size):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        blk = data[at:at + block_size]
        payload = c.compress(blk) + c.flush()
        if not payload[0] & 1:          # zlib cut the bytes into several DEFLATE blocks: one stored block instead
            payload = b"\x01" + struct.pack("<HH", len(blk), len(blk) ^ 0xFFFF) + blk
        out.append(bgzf.frame(payload, blk))
    return b"".join(out)


def bam_file(header: bytes, recs, block_size: int, chunk_ends=()):
    """a BAM file: the header in blocks of its own, the records (already sorted) cut into chunks behind records chunk_ends, every chunk in
    blocks of its own, the end-of-file block.  Returns (file, [(first record, end record, the chunk's bytes, file offset)])."""
    out = deflate_blocks(bam.encode_header(header), block_size)
    chunks, a = [], 0
    for b in list(chunk_ends) + [len(recs)]:
        if b > a:
            data = b"".join(recs[a:b])
            chunks.append((a, b, data, len(out)))
            out += deflate_blocks(data, block_size)
            a = b
    return out + bgzf.EOF_BLOCK, chunks


def block_sizes(blocks: bytes):
    """the compressed size of every block, from BSIZE"""
    out, at = [], 0
    while at < len(blocks):
        out.append(struct.unpack_from("<H", blocks, at + 16)[0] + 1)
        at += out[-1]
    return out


def ents_of(recs) -> list:
    """the index entries of records in stream order, as moni_bam_ent_t has them"""
    out, at = [], 0
    for r in recs:
        ref, pos, end, bin_, flag = bsm.fields(r)
        out.append((ref, pos, end, bin_ << 16 | flag, at))
        at += len(r)
    return out
