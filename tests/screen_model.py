"""Read screening in plain Python on top of tests/pml_model.PmlModel: the definition of DESIGN.md 7.10, written for reading, not for speed.
Every read is walked as four strings - P0 the bytes as they are, P1 the reverse complement by the index's table, N0 and N1 their reverses - and
windows of pseudo-matching lengths of a pattern are compared with those of its null by the one-sided Kolmogorov-Smirnov numerator.  The
yardstick of the screening tests; render() is the text of `moni-hip-align --screen`."""
from collections import namedtuple

import numpy as np

BINS = 32
PRESENT, STRAND1, SHORT = 1, 2, 4

Params = namedtuple("Params", "window min_win ks_num ks_den strands", defaults=(50, 25, 1, 4, 2))

# the complement table of image.hpp (kpbseq.h:120-137): A <-> T, C <-> G, lower case to the upper-case complement, every other byte to itself
COMPL = np.arange(256, dtype=np.uint8)
for _a, _b in (("A", "T"), ("C", "G"), ("G", "C"), ("T", "A")):
    COMPL[ord(_a)] = COMPL[ord(_a.lower())] = ord(_b)


def params_ok(p: Params) -> bool:
    return 8 <= p.window <= 65535 and 1 <= p.min_win <= p.window and 1 <= p.ks_num <= p.ks_den <= 65535 and p.strands in (1, 2)


def windows(m: int, p: Params):
    """(start, end) of the scored windows of a read of m offsets"""
    out = []
    for j in range((m + p.window - 1) // p.window):
        lo, hi = j * p.window, min(m, (j + 1) * p.window)
        if hi - lo == p.window or hi - lo >= p.min_win:
            out.append((lo, hi))
    return out


def ks_d(a, b) -> int:
    """max over v in 0 .. BINS-2 of #{b <= v} - #{a <= v}, lengths clipped to BINS-1: an integer in 0 .. len (at v = BINS-1 both counts are
    len and the difference 0, so a maximum below 0 reads 0: the one-sided statistic over every v)"""
    ha, hb = [0] * BINS, [0] * BINS
    for x in a:
        ha[min(int(x), BINS - 1)] += 1
    for x in b:
        hb[min(int(x), BINS - 1)] += 1
    d = cum = 0
    for v in range(BINS - 1):
        cum += hb[v] - ha[v]
        d = max(d, cum)
    return d


def strand_patterns(read: bytes, p: Params, compl=COMPL):
    pats = [read]
    if p.strands == 2:
        pats.append(bytes(compl[np.frombuffer(read, dtype=np.uint8)][::-1].tolist()))
    return pats


def walk_read(model, read: bytes, strands: int = 2, compl=COMPL):
    """per strand (a_s, b_s): the pseudo-matching lengths of Ps and of its null reverse(Ps), each indexed by offset in its own string"""
    return [(model.query(pat), model.query(pat[::-1])) for pat in strand_patterns(read, Params(strands=strands), compl)]


def screen_read(model, read: bytes, p: Params = Params(), compl=COMPL, walked=None):
    """the record of one read: (n_win, (n_pos0, n_pos1), (d_max0, d_max1), (max_pml0, max_pml1), flags); walked: walk_read's answer for the
    read (both strands), where the caller scores one walk under several parameter sets"""
    assert params_ok(p)
    m = len(read)
    wins = windows(m, p)
    n_pos, d_max, mx = [0, 0], [0, 0], [0, 0]
    if walked is None:
        walked = walk_read(model, read, p.strands, compl)
    for s, (a, b) in enumerate(walked[:p.strands]):
        mx[s] = max(a) if a else 0
        for lo, hi in wins:
            d = ks_d(a[lo:hi], b[lo:hi])
            d_max[s] = max(d_max[s], d)
            if d * p.ks_den >= p.ks_num * (hi - lo):
                n_pos[s] += 1
    n_win = len(wins)
    flags = 0
    if 2 * n_pos[0] > n_win or 2 * n_pos[1] > n_win:
        flags |= PRESENT
    if n_pos[1] > n_pos[0]:
        flags |= STRAND1
    if n_win == 0:
        flags |= SHORT
    return (n_win, tuple(n_pos), tuple(d_max), tuple(mx), flags)


def screen_batch(model, reads, p: Params = Params(), compl=COMPL):
    return [screen_read(model, r, p, compl) for r in reads]


def as_tuples(res):
    """records of capi.SCREEN_RES_DTYPE as the tuples of screen_read"""
    return [(int(r["n_win"]), tuple(int(x) for x in r["n_pos"]), tuple(int(x) for x in r["d_max"]), tuple(int(x) for x in r["max_pml"]), int(r["flags"])) for r in res]


def n_present(recs) -> int:
    return sum(1 for r in recs if r[4] & PRESENT)


def render(names, reads, recs) -> bytes:
    """<out>.screen: name, length, P|A|S, +|-|. , n_win, n_pos0, n_pos1, d_max0, d_max1, max_pml0, max_pml1 - tab-separated, one line per read"""
    out = []
    for name, read, (n_win, n_pos, d_max, mx, flags) in zip(names, reads, recs):
        call = b"S" if flags & SHORT else (b"P" if flags & PRESENT else b"A")
        strand = b"." if not flags & PRESENT else (b"-" if flags & STRAND1 else b"+")
        out.append(b"\t".join([name, b"%d" % len(read), call, strand] + [b"%d" % x for x in (n_win, n_pos[0], n_pos[1], d_max[0], d_max[1], mx[0], mx[1])]) + b"\n")
    return b"".join(out)
