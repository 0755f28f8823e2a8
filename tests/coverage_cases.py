"""Inputs of the coverage tests (tests/test_host_coverage.py on the CPU, tests/test_gpu_coverage.py on the GPU): the smallest shapes at which
the kernels of DESIGN.md 7.17 can go wrong, over a dictionary of three references of 1, 70 and 200 bases.  TEST HARNESS."""
import struct

import numpy as np

from tests.bamsort_cases import record

HDR = b"@HD\tVN:1.6\tSO:unknown\n@SQ\tSN:a\tLN:1\n@SQ\tSN:chrB\tLN:70\n@SQ\tSN:c\tLN:200\n"
LN = (1, 70, 200)
H_ONE = b"@HD\tVN:1.6\tSO:unknown\n@SQ\tSN:chr1\tLN:100\n"          # for the bad-record classes of tests/bamsort_cases: one reference
MAPQ_THRESHOLD = 20          # of the cases run with a threshold
BASES_GRID = (1, 7, 64, 1 << 20)
LINES_GRID = (1, 2, 3, 1 << 20)
WINDOWS = (1, 16, 70, 1000)


def rec(ref=1, pos=0, ops=((10, "M"),), flag=0, mapq=30, seed=0) -> bytes:
    r = record(ref=ref, pos=pos, flag=flag, ops=list(ops), name=b"q%d" % seed, l_seq=4, seed=seed)
    return r[:13] + struct.pack("<B", mapq) + r[14:]


def _random(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ref = int(rng.integers(-1, 3))
        ln = LN[ref] if ref >= 0 else 50
        ops = [(int(rng.integers(0, 40)), "MIDNSHP=X"[int(rng.integers(0, 9))]) for _ in range(int(rng.integers(0, 6)))]
        flag = int(rng.integers(0, 65536)) if rng.random() < 0.3 else int(rng.integers(0, 2)) * 16 | int(rng.integers(0, 2)) * 0x800
        out.append(rec(ref=ref, pos=int(rng.integers(-1, ln + 5)) if ref >= 0 else -1, ops=ops, flag=flag, mapq=int(rng.integers(0, 61)), seed=i))
    return out


def cases():
    """(name, [records], min_mapq)"""
    c = []
    c.append(("n0", [], 0))
    c.append(("edges", [rec(ref=1, pos=0, ops=[(5, "M")]),                       # at pos 0
                        rec(ref=1, pos=60, ops=[(10, "M")], seed=1),             # ends exactly at LN
                        rec(ref=1, pos=65, ops=[(10, "M")], seed=2),             # reaches past LN: clipped
                        rec(ref=1, pos=69, ops=[(1, "M")], seed=3),              # starts at LN - 1
                        rec(ref=1, pos=69, ops=[(9, "M")], seed=4),              # ... and is clipped
                        rec(ref=0, pos=0, ops=[(1, "M")], seed=5),               # the reference of one base
                        rec(ref=0, pos=0, ops=[(3, "M")], seed=6),
                        rec(ref=2, pos=199, ops=[(1, "M"), (5, "N"), (3, "M")], seed=7),      # second block dropped
                        rec(ref=2, pos=0, ops=[(200, "M")], seed=8)], 0))
    c.append(("cigars", [rec(ref=2, pos=10, ops=[(5, "M"), (3, "D"), (4, "M")]),
                         rec(ref=2, pos=10, ops=[(5, "M"), (30, "N"), (4, "M")], seed=1),
                         rec(ref=2, pos=12, ops=[(5, "M"), (7, "I"), (4, "M")], seed=2),
                         rec(ref=2, pos=20, ops=[(3, "S"), (6, "M"), (2, "S")], seed=3),
                         rec(ref=2, pos=20, ops=[(3, "H"), (6, "M"), (2, "H")], seed=4),
                         rec(ref=2, pos=30, ops=[(4, "M"), (2, "P"), (4, "M")], seed=5),
                         rec(ref=2, pos=40, ops=[(4, "="), (1, "X"), (4, "=")], seed=6),
                         rec(ref=2, pos=50, ops=[(4, "M"), (9, "N")], seed=7),               # N as the last operation
                         rec(ref=2, pos=190, ops=[(4, "M"), (9, "N"), (2, "M")], seed=8),    # ... and a block behind LN after it
                         rec(ref=2, pos=60, ops=[(4, "N"), (3, "M")], seed=9),
                         rec(ref=2, pos=70, ops=[(2, "M"), (1, "N"), (2, "M"), (1, "N"), (2, "M"), (1, "N"), (2, "M"), (1, "N"), (2, "M")], seed=10),
                         rec(ref=2, pos=80, ops=[(5, "S"), (6, "I")], seed=11),              # no covering operation
                         rec(ref=2, pos=90, ops=[(0, "M")], seed=12),
                         rec(ref=2, pos=5, ops=[], seed=13),                                  # mapped, CIGAR *
                         rec(ref=-1, pos=-1, ops=[], flag=4, seed=14),
                         rec(ref=-1, pos=-1, ops=[(5, "M")], seed=15),
                         rec(ref=1, pos=-1, ops=[(5, "M")], seed=16)], 0))
    c.append(("flags", [rec(ref=1, pos=3 * i, ops=[(10, "M")], flag=f, seed=i) for i, f in enumerate((0, 0x4, 0x100, 0x200, 0x400, 0x800, 0x10, 0x1, 0x704, 0xF8FB))], 0))
    c.append(("mapq", [rec(ref=1, pos=5 * i, ops=[(10, "M")], mapq=q, seed=i) for i, q in enumerate((MAPQ_THRESHOLD, MAPQ_THRESHOLD - 1, MAPQ_THRESHOLD + 1, 0, 255))] +
              [rec(ref=1, pos=1, ops=[(4, "M")], mapq=0, flag=0x400, seed=9), rec(ref=-1, pos=-1, ops=[], mapq=0, flag=0x400, seed=10)], MAPQ_THRESHOLD))
    c.append(("pile65", [rec(ref=1, pos=33, ops=[(1, "M")], seed=i) for i in range(65)], 0))
    c.append(("pile257", [rec(ref=2, pos=100 - i % 3, ops=[(2 + i % 5, "M")], seed=i) for i in range(257)], 0))
    # the same depth on both sides of both boundaries: the line must break there
    c.append(("boundary", [rec(ref=0, pos=0, ops=[(1, "M")]), rec(ref=1, pos=0, ops=[(70, "M")], seed=1), rec(ref=2, pos=0, ops=[(9, "M")], seed=2)], 0))
    c.append(("empty_ref", [rec(ref=0, pos=0, ops=[(1, "M")]), rec(ref=2, pos=3, ops=[(9, "M")], seed=1)], 0))
    c.append(("random3000", _random(3000, 5), 0))
    c.append(("random3000_mapq", _random(3000, 6), MAPQ_THRESHOLD))
    return c
