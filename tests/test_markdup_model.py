"""tests/markdup_model against answers worked out by hand: twelve records (six pairs) whose end codes, scores and decisions stand in the text
below, the single-end rule on a second small set, and the three bad-record reasons."""
import struct

import pytest

from tests import markdup_model as md
from tests.bamsort_cases import H1
from tests.markdup_cases import line, pair, records

B = 2 ** 31


def e(u5, rev, ref=0):
    return ref << 34 | (u5 + B) << 1 | rev


def test_twelve_records_by_hand():
    lines = (
        # A: read 1 forward at 100, 50M: u5 100, score 50 * 30 = 1500.  Read 2 reverse at 300, 50M: u5 300 + 50 - 1 = 349, score 1500.
        pair("A", 100, 0, 300, 16, q=30)
        # B: read 1 forward at 105, 5S45M: u5 105 - 5 = 100, score 50 * 31 = 1550.  Read 2 reverse at 300, 45M5H, 45 bases: u5 300 + 45 - 1 + 5 = 349,
        # score 45 * 31 = 1395.  The ends of A, the score 2945 < 3000: both records are duplicates.
        + [line("B", 0x61, 105, "5S45M", 50, 31), line("B", 0x91, 300, "45M5H", 45, 31)]
        # C: read 1 reverse at 51: u5 100 reverse; read 2 forward at 349.  Positions of A's ends, other strands: other codes, no duplicate.
        + pair("C", 51, 16, 349, 0, q=40)
        # D: read 1 forward at 100 with qualities of 14 (score 0), its mate unmapped: a fragment at an end of A and B - a duplicate whatever it scores.
        + [line("D", 0x49, 100, q=14), line("D", 0x85, 100, "*")]
        # E: read 1 forward at 700, qualities of 15: score 750, the mate unmapped.  F: read 1 unmapped, read 2 forward at 700, score 750.
        # No pair ends at (700, forward): the better fragment stays, at a tie the earlier - E stays, F's read 2 is a duplicate.
        + [line("E", 0x49, 700, q=15), line("E", 0x85, 700, "*")]
        + [line("F", 0x45, 700, "*"), line("F", 0x89, 700, q=15)]
    )
    recs = records(H1, lines)
    assert len(recs) == 12
    sigs = [md.signature(r, 1) for r in recs]
    assert sigs[0] == (True, e(100, 0), 1500) and sigs[1] == (True, e(349, 1), 1500)
    assert sigs[2] == (True, e(100, 0), 1550) and sigs[3] == (True, e(349, 1), 1395)
    assert sigs[4] == (True, e(100, 1), 2000) and sigs[5] == (True, e(349, 0), 2000)
    assert sigs[6] == (True, e(100, 0), 0) and sigs[7] == (False, 0, 0)
    assert sigs[8] == (True, e(700, 0), 750) and sigs[10] == (False, 0, 0) and sigs[11] == (True, e(700, 0), 750)
    assert e(100, 0) == (100 + B) * 2 and e(349, 1) == (349 + B) * 2 + 1 and e(5, 0, ref=3) == 3 << 34 | (5 + B) << 1
    ents = md.entries(recs, True, 1)
    assert ents == [
        (e(100, 0), e(349, 1), 3000, 1, (0, 1)),
        (e(100, 0), e(349, 1), 2945, 1, (2, 3)),
        (e(100, 1), e(349, 0), 4000, 1, (4, 5)),
        (e(100, 0), 0, 0, 0, (6, None)),
        (e(700, 0), 0, 750, 0, (8, None)),
        (e(700, 0), 0, 750, 0, (11, None)),
    ]
    marked = md.resolve([ents])
    assert marked == {(0, 2), (0, 3), (0, 6), (0, 11)}
    assert md.counts([ents], marked) == (3, 1, 3, 2, 4)
    # the same entries split over two runs: input order is run order
    assert md.resolve([ents[:2], ents[2:]]) == {(0, 2), (0, 3), (1, 6), (1, 11)}
    # a better B in an earlier run: A becomes the duplicate
    better = [(e(100, 0), e(349, 1), 3001, 1, (0, 1))]
    assert md.resolve([better, ents]) == {(1, 0), (1, 1), (1, 2), (1, 3), (1, 6), (1, 11)}
    flagged = md.set_flags(recs, [i for _, i in marked])
    assert [struct.unpack_from("<H", r, 18)[0] & 0x400 for r in flagged] == [0, 0, 0x400, 0x400, 0, 0, 0x400, 0, 0, 0, 0, 0x400]
    assert all(a[:18] == b[:18] and a[20:] == b[20:] and len(a) == len(b) for a, b in zip(recs, flagged))


def test_kinds_and_ties():
    # FF: read 1 at 100 and read 2 at 400 (lo is read 1, kind 1) against read 1 at 400 and read 2 at 100 (lo is read 2, kind 3): not duplicates
    recs = records(H1, pair("x", 100, 0, 400, 0) + pair("y", 400, 0, 100, 0) + pair("z", 100, 0, 100, 0) + pair("w", 100, 0, 100, 0, q=29))
    ents = md.entries(recs, True, 1)
    assert [k for _, _, _, k, _ in ents] == [1, 3, 1, 1]          # e1 == e2: lo is read 1
    assert ents[0][:2] == ents[1][:2] == (e(100, 0), e(400, 0))
    assert md.resolve([ents]) == {(0, 6), (0, 7)}          # w behind z alone


def test_single_end_by_hand():
    lines = [line("a", 0, 10, q=20), line("b", 0, 10, q=22), line("c", 16, 10, q=20), line("d", 0, 10, q=22), line("u", 4, 10, "*"),
             line("s", 0x100, 10), line("t", 0x800, 10), line("k", 16, 0, "*", 0), line("h", 0, 0, "4S3H", 4)]
    recs = records(H1, lines)
    ents = md.entries(recs, False, 1)
    # a, b, d at (10, forward) with 1000, 1100, 1100: b stays.  c at (10 + 49, reverse) alone.  u, s, t take no part.
    # k: no ops on the reverse strand, u5 = 0 + 0 - 1 = -1.  h: clips only, u5 = 0 - 7.
    assert [(x[0], x[2], x[4][0]) for x in ents] == [(e(10, 0), 1000, 0), (e(10, 0), 1100, 1), (e(59, 1), 1000, 2), (e(10, 0), 1100, 3), (e(-1, 1), 0, 7), (e(-7, 0), 120, 8)]
    assert md.resolve([ents]) == {(0, 0), (0, 3)}
    assert md.sorted_places(recs, 1)[7:] == [1, 0] and md.pack_entries(ents[:1], md.sorted_places(recs, 1))[24:32] == struct.pack("<II", md.sorted_places(recs, 1)[0], md.NONE)


def test_bad_records():
    good = records(H1, pair("n0", 0, 0, 200, 16) + pair("n1", 10, 0, 210, 16) + pair("n2", 20, 0, 220, 16))
    short = good[2][:20] + struct.pack("<I", 200) + good[2][24:]          # l_seq of 200 in a record that holds 50
    with pytest.raises(md.MarkdupError) as x:
        md.entries(good[:2] + [short] + good[3:], True, 1)
    assert (x.value.reason, x.value.index) == (md.SEQ, 2)
    huge = records(H1, [line("n1", 0x61, 0, "268435455H" * 40 + "5M", 5)])[0]
    with pytest.raises(md.MarkdupError) as x:
        md.entries(good[:2] + [huge] + good[3:], True, 1)
    assert (x.value.reason, x.value.index, x.value.count) == (md.CLIP, 2, 1)
    for bad in (good[:3] + [good[2]] + good[4:], good[:3] + records(H1, [line("zz", 0x91, 210)]) + good[4:], good[:5]):
        with pytest.raises(md.MarkdupError) as x:
            md.entries(bad, True, 1)
        assert x.value.reason == md.MATE and x.value.index == (4 if len(bad) == 5 else 2)
    assert len(md.entries(good[:5], False, 1)) == 5          # single-end: an odd number is fine
    # u5 at the edges of the range
    assert md.signature(records(H1, [line("r", 0, 0, "268435455H" * 8 + "8H1M", 1)])[0], 1)[1] == e(-B, 0)
    with pytest.raises(md.MarkdupError):
        md.signature(records(H1, [line("r", 0, 0, "268435455H" * 8 + "9H1M", 1)])[0], 1)
