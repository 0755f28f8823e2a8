"""tests/coverage_model against a counter that visits every base of every record, and against lines written by hand."""
import struct

import numpy as np
import pytest

from tests import bam_model as bam
from tests import coverage_model as cm
from tests.coverage_cases import HDR, LN, cases, rec

CASES = cases()


def brute(recs, exclude, min_mapq):
    """depth per reference, one base at a time, from the record's fields read here"""
    depth = [[0] * ln for ln in LN]
    for r in recs:
        ref, pos, l_name, mapq, _, n_ops, flag = struct.unpack_from("<iiBBHHH", r, 4)
        if ref < 0 or pos < 0 or n_ops == 0 or flag & exclude or mapq < min_mapq:
            continue
        p = pos
        for k in range(n_ops):
            v = struct.unpack_from("<I", r, 36 + l_name + 4 * k)[0]
            op, n = "MIDNSHP=X"[v & 15], v >> 4
            if op in "M=XD":
                for x in range(p, p + n):
                    if x < LN[ref]:
                        depth[ref][x] += 1
            if op in "M=XDN":
                p += n
    return depth


@pytest.mark.parametrize("name,recs,mapq", CASES, ids=[c[0] for c in CASES])
def test_model_matches_brute_force(name, recs, mapq):
    m = cm.Coverage(HDR, min_mapq=mapq).add(recs)
    want = brute(recs, cm.EXCLUDE, mapq)
    for r in range(3):
        assert m.depth(r).tolist() == want[r]
    # the text spells the same depths: expand it again
    got = [[None] * ln for ln in LN]
    names = [n for n, _ in bam.references(HDR)]
    last = None
    for line in m.per_base().splitlines():
        n, a, b, d = line.split(b"\t")
        r, a, b, d = names.index(n), int(a), int(b), int(d)
        assert a < b
        if last is not None and last[0] == r:
            assert last[1] == a and last[2] != d, "runs are maximal and follow one another"
        else:
            assert a == 0
        for x in range(a, b):
            got[r][x] = d
        last = (r, b, d)
    assert got == want
    assert m.stats["records"] == len(recs) and sum(m.stats[k] for k in ("counted", "skipped_flag", "skipped_mapq", "unplaced")) == len(recs)
    for r in range(3):
        for w in (1, 16, 70, 1000):
            assert m.windows(r, w) == [sum(want[r][a:a + w]) for a in range(0, LN[r], w)]


def test_excluding_other_flags_changes_the_depth():
    recs = [rec(pos=0, ops=[(4, "M")], flag=0x400), rec(pos=2, ops=[(4, "M")], seed=1)]
    assert cm.Coverage(HDR).add(recs).depth(1)[:7].tolist() == [0, 0, 1, 1, 1, 1, 0]
    assert cm.Coverage(HDR, exclude=0x304).add(recs).depth(1)[:7].tolist() == [1, 1, 2, 2, 1, 1, 0]


def test_golden_text():
    recs = [rec(ref=1, pos=2, ops=[(3, "M"), (2, "D"), (1, "M")]), rec(ref=1, pos=4, ops=[(2, "M"), (10, "N"), (2, "M")], seed=1),
            rec(ref=1, pos=68, ops=[(5, "M")], seed=2), rec(ref=0, pos=0, ops=[(1, "M")], seed=3)]
    m = cm.Coverage(HDR).add(recs)
    assert m.per_base() == (b"a\t0\t1\t1\n"
                            b"chrB\t0\t2\t0\nchrB\t2\t4\t1\nchrB\t4\t6\t2\nchrB\t6\t8\t1\nchrB\t8\t16\t0\nchrB\t16\t18\t1\nchrB\t18\t68\t0\nchrB\t68\t70\t1\n"
                            b"c\t0\t200\t0\n")
    assert m.stats == dict(records=4, counted=4, skipped_flag=0, skipped_mapq=0, unplaced=0, clipped=1, blocks=5)
    assert m.summary() == (b"chrom\tlength\tbases\tmean\tmin\tmax\n"
                           b"a\t1\t1\t1.00\t1\t1\nchrB\t70\t12\t0.17\t0\t2\nc\t200\t0\t0.00\t0\t0\ntotal\t271\t13\t0.05\t0\t2\n")
    assert m.windows(1, 16) == [8, 2, 0, 0, 2]
    assert m.regions(50) == b"a\t0\t1\t1.00\nchrB\t0\t50\t0.20\nchrB\t50\t70\t0.10\nc\t0\t50\t0.00\nc\t50\t100\t0.00\nc\t100\t150\t0.00\nc\t150\t200\t0.00\n"


def test_golden_classes():
    recs = [rec(flag=0x4), rec(flag=0x800, seed=1), rec(mapq=3, seed=2), rec(ref=-1, pos=-1, ops=[], flag=0x400, mapq=0, seed=3), rec(ops=[], seed=4)]
    m = cm.Coverage(HDR, min_mapq=10).add(recs)
    assert m.stats == dict(records=5, counted=1, skipped_flag=1, skipped_mapq=1, unplaced=2, clipped=0, blocks=1)


def test_of_bam_file():
    from tests.bamsort_cases import bam_file
    recs = [rec(ref=1, pos=2, ops=[(3, "M")]), rec(ref=2, pos=4, ops=[(2, "M")], seed=1)]
    data, _ = bam_file(HDR, recs, 65280)
    assert cm.of_bam_file(data).per_base() == cm.Coverage(HDR).add(recs).per_base()
