"""Inputs of the duplicate-marking tests (tests/test_host_markdup.py on the CPU, tests/test_gpu_markdup.py on the GPU): SAM lines written field by
field - the library's run call takes SAM text -, the issue's case list as runs of such lines, and the bad-record classes.  TEST HARNESS."""
import numpy as np

from tests import bam_model as bam
from tests import bamsort_model as bsm
from tests.bamsort_cases import H1, H2

M50 = "50M"


def line(name, flag, pos, cigar=M50, l_seq=50, q=30, ref="chr1") -> bytes:
    """one SAM line; pos is 0-based as in the record (-1: none); q: one Phred value, a list of them, or None for a missing QUAL"""
    seq = "A" * l_seq if l_seq else "*"
    if q is None or not l_seq:
        qual = "*"
    else:
        qs = [q] * l_seq if isinstance(q, int) else list(q)
        assert len(qs) == l_seq
        qual = "".join(chr(33 + x) for x in qs)
    return ("%s\t%d\t%s\t%d\t30\t%s\t*\t0\t0\t%s\t%s\n" % (name, flag, ref, pos + 1, cigar, seq, qual)).encode()


def pair(name, p1, s1, p2, s2, q=30, c1=M50, c2=M50, ref1="chr1", ref2="chr1", l_seq=50, q2=None):
    """both mates mapped: read 1 at p1 on strand s1 (0 / 16), read 2 at p2 on s2"""
    return [line(name, 0x41 | s1 | s2 << 1, p1, c1, l_seq, q, ref1), line(name, 0x81 | s2 | s1 << 1, p2, c2, l_seq, q if q2 is None else q2, ref2)]


def records(header: bytes, lines) -> list:
    return bsm.split_records(bam.encode_records(header, b"".join(lines)))


def _units(n, paired):
    out = []
    for i in range(n):
        pos = (i * 7919) % 5 * 10
        if not paired:
            out.append(line("r%d" % i, 0 if i % 3 else 16, pos, l_seq=i % 70 + 1, cigar="%dM" % (i % 70 + 1), q=20 + i % 7))
        elif i % 4 == 3:          # the second mate unmapped
            out += [line("p%d" % i, 0x49, pos), line("p%d" % i, 0x85, pos, cigar="*")]
        else:
            out += pair("p%d" % i, pos, 0, pos + 100 + i % 3, 16, q=25 + i % 5)
    return out


def _random(n, seed, n_runs):
    """n units from 50 end codes (5 positions, 2 strands, 5 clips that fold onto the positions), so that the groups are large"""
    rng = np.random.default_rng(seed)
    runs = [[] for _ in range(n_runs)]
    for i in range(n):
        def one():
            p, s, clip = int(rng.integers(0, 5)) * 40 + 100, int(rng.integers(0, 2)) * 16, int(rng.integers(0, 5))
            cig = ("%dS%dM" % (clip, 50 - clip) if clip else M50) if not s else ("%dM%dH" % (50 - clip, clip) if clip else M50)
            return p + (clip if not s else 0), s, cig, int(rng.integers(20, 24))
        (p1, s1, c1, q1), (p2, s2, c2, q2) = one(), one()
        kind = int(rng.integers(0, 8))
        if kind == 0:
            u = [line("u%d" % i, 0x49 | s1, p1, c1, q=q1), line("u%d" % i, 0x85 | s1 << 1, p1, "*", q=q2)]
        elif kind == 1:
            u = [line("u%d" % i, 0x4D, -1, "*", ref="*"), line("u%d" % i, 0x8D, -1, "*", ref="*")]
        else:
            u = pair("u%d" % i, p1, s1, p2, s2, q=q1, c1=c1, c2=c2, q2=q2)
        runs[i * n_runs // n] += u
    return runs


def cases():
    """(name, header, paired, [runs of lines]) - the issue's list"""
    c = []
    for n in (0, 1, 2, 63, 64, 65, 257):
        c.append(("se_n%d" % n, H2, False, [_units(n, False)]))
        c.append(("pe_n%d" % n, H2, True, [_units(n, True)]))
    c.append(("clips", H1, False, [[
        line("a", 0, 105, "5S45M"), line("b", 0, 100, q=40), line("c", 0, 107, "3H4S43M", q=20),                # u5 100 forward: b stays
        line("d", 16, 100, "45M5H", l_seq=45), line("e", 16, 100, "2H50M", q=20), line("f", 16, 110, "30M4S6H", l_seq=34),          # u5 149 reverse
        line("g", 0, 3, "10S40M"), line("h", 0, 0, "4S3H", l_seq=4), line("i", 0, -1, "6S", l_seq=6),          # u5 -7: clips before pos 0, clips only
        line("j", 0, 0, "*", l_seq=0), line("k", 16, 0, "*", l_seq=0),                                          # no ops: u5 0 forward, -1 reverse
        line("l", 16, 2 ** 31 - 3, "1M9S", l_seq=10), line("m", 16, 2 ** 31 - 3, "1M9S", l_seq=10, q=20),   # u5 beyond the reference's end
        line("n", 0, 100, "2I48M"),                                                                              # an I is no clip: u5 100
    ]]))
    c.append(("lengths", H1, False, [[line("s%d_%d" % (n, k), 0, 500, "%dM" % max(n, 1), n, 20 + k) for n in (0, 1, 63, 64, 65, 300) for k in (0, 1)]]))
    c.append(("qualities", H1, False, [[
        line("q0", 0, 7, l_seq=64, q=[14, 15] * 32), line("q1", 0, 7, l_seq=64, q=None), line("q2", 0, 7, l_seq=1, cigar="1M", q=15),
        line("q3", 0, 7, l_seq=33, cigar="33M", q=14), line("q4", 0, 7, l_seq=33, cigar="33M", q=[15] + [14] * 32), line("q5", 0, 7, l_seq=5, cigar="5M", q=93),
    ]]))
    c.append(("pairs", H2, True, [
        pair("p0", 100, 0, 300, 16) + pair("p1", 100, 0, 300, 16)           # equal scores: the first stays
        + pair("p2", 51, 16, 349, 0)                                         # RF at the ends of FR: other codes
        + pair("p3", 100, 0, 400, 0) + pair("p4", 400, 0, 100, 0)           # FF, lo read 1 against lo read 2
        + pair("p5", 100, 0, 300, 16, ref2="chr2") + pair("p6", 100, 0, 300, 16, ref2="chr2", q=31)          # mates on different references
        + pair("p7", 100, 0, 100, 0) + pair("p8", 100, 0, 100, 0, q=31) + pair("p9", 149, 16, 149, 16),       # e1 == e2
        pair("p10", 300, 16, 100, 0, q=35)                                   # read 2 forward at 100, read 1 reverse at 300: FR again, better, in the next run
        + [line("f0", 0x49, 100, q=40), line("f0", 0x85, 100, "*")]         # a fragment at a pair's end, whatever its score
        + [line("f1", 0x4D, -1, "*", ref="*"), line("f1", 0x8D, -1, "*", ref="*")]          # both unmapped
        + [line("f2", 0x45, 700, "*"), line("f2", 0x99, 700)]               # read 1 unmapped
        + [line("f3", 0x141, 100), line("f3", 0x881, 300)]                   # secondary, supplementary: no entries
        + [line("f4", 4, -1, "*", ref="*"), line("f4", 4, -1, "*", ref="*")],          # an unaligned pair as the aligner writes it: flag 4 twice
    ]))
    c.append(("fragments", H1, False, [
        [line("g0", 0, 10, q=20), line("g1", 0, 10, q=22), line("g2", 16, 10, q=20), line("g3", 0, 10, q=22), line("g4", 4, 10, "*"), line("g5", 0x100, 10), line("g6", 0x800, 10)],
        [],
        [line("g7", 0, 10, q=21), line("g8", 16, 10, q=25), line("g9", 0, 11)],
    ]))
    c.append(("runs_2", H2, True, _random(300, 3, 2)))
    c.append(("runs_7", H2, True, _random(700, 4, 7)[:3] + [[]] + _random(700, 4, 7)[3:]))
    c.append(("all_runs_empty", H2, True, [[], [], []]))
    c.append(("random2000", H2, True, _random(2000, 5, 4)))
    return c


def bad_runs():
    """(name, paired, lines, reason, first bad record, bad records / units): at unit 2 of 6 and again at unit 4, which the replay meets first"""
    good = [pair("n%d" % i, 10 * i, 0, 10 * i + 200, 16) for i in range(6)]
    huge = "".join(["268435455H"] * 40) + "5M"

    def with_(f):
        units = [list(u) for u in good]
        for k in (2, 4):
            units[k] = f(units[k], k)
        return [x for u in units for x in u]
    out = [
        ("clip", True, with_(lambda u, k: [line("n%d" % k, 0x61, 0, huge, 5), u[1]]), "CLIP", 4, 2),
        ("mate_flag", True, with_(lambda u, k: [u[0], u[1].replace(b"\t145\t", b"\t81\t")]), "MATE", 4, 2),
        ("mate_both_first", True, with_(lambda u, k: [u[0].replace(b"\t97\t", b"\t225\t"), u[1]]), "MATE", 4, 2),
        ("mate_name", True, with_(lambda u, k: [u[0], b"x" + u[1]]), "MATE", 4, 2),
        ("odd_n", True, [x for u in good for x in u][:-1], "MATE", 10, 1),
        ("clip_single", False, with_(lambda u, k: [line("n%d" % k, 16, 2 ** 31 - 10, "5M" + huge[:-2], 5), u[1]]), "CLIP", 4, 2),
    ]
    return out
