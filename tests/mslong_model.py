"""What the tests of moni_ms_long_batch share (tests/test_host_mslong.py replays the per-lane code on the host, tests/test_gpu_mslong.py runs the
kernels): a plain-Python restatement of the segment cuts, the patterns the issue lists, the prediction of which segments are flagged from the
oracle's matching statistics alone, and the checks, none of which has a tolerance.

A `runner` is any callable (seq, offs, seg_len, overlap) -> (pointers, lengths, stats) with stats holding segments, flagged, chain_runs,
steps_spec, steps_chain."""
import numpy as np

SETTINGS = [(8, 0), (8, 3), (16, 8), (64, 16), (4096, 256)]
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def cuts(g0: int, m: int, seg_len: int, overlap: int):
    """[(a, b, e)] of a pattern of m bases whose first output index is g0 (csrc/mslong_core.h: seg_len down to a multiple of 8, the first
    segment shortened so that the later ones begin at a multiple of 8 of the output index; at most seg_len bases: one segment)"""
    if m == 0:
        return []
    if m <= seg_len:
        return [(0, m, m)]
    sl8 = seg_len - seg_len % 8
    bounds = [0]
    at = sl8 - g0 % 8
    while at < m:
        bounds.append(at)
        at += sl8
    bounds.append(m)
    return [(a, b, min(b + overlap, m)) for a, b in zip(bounds[:-1], bounds[1:])]


def table(pats, seg_len, overlap):
    """[(pattern, a, b, e)] of a batch, in the library's order"""
    out, g0 = [], 0
    for i, p in enumerate(pats):
        out += [(i, a, b, e) for a, b, e in cuts(g0, len(p), seg_len, overlap)]
        g0 += len(p)
    return out


def ragged(pats):
    offs = np.zeros(len(pats) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(p) for p in pats])
    seq = np.frombuffer(b"".join(pats), dtype=np.uint8).copy() if int(offs[-1]) else np.zeros(0, np.uint8)
    return seq, offs


def predict(pats, want_len, seg_len, overlap):
    """From the matching statistics alone: a segment with e < m is flagged iff (b - 1) + MS[b - 1] >= e.  Returns the table, the flags, the number of
    runs of flagged neighbours, steps_spec and steps_chain."""
    tab = table(pats, seg_len, overlap)
    flags = [e < len(pats[i]) and (b - 1) + int(want_len[i][b - 1]) >= e for i, a, b, e in tab]
    runs = sum(1 for k, f in enumerate(flags) if f and (k == 0 or not flags[k - 1]))
    steps_spec = sum(len(p) for p in pats) + sum(e - b for _, a, b, e in tab)
    steps_chain = sum(b - a for (_, a, b, e), f in zip(tab, flags) if f)
    return tab, flags, runs, steps_spec, steps_chain


def check(runner, oracle, text: bytes, n: int, pats, seg_len, overlap, want=None):
    """Runs the batch and holds it to the oracle; returns (stats, prediction, oracle results).  want: [(pointers, lengths)] of the oracle per
    pattern, when the caller has them already."""
    if want is None:
        want = [oracle.ms_lengths(p) for p in pats]
    seq, offs = ragged(pats)
    ptr, ln, st = runner(seq, offs, seg_len, overlap)
    tab, flags, runs, steps_spec, steps_chain = predict(pats, [w[1] for w in want], seg_len, overlap)
    for i, p in enumerate(pats):
        o, m = int(offs[i]), len(p)
        gl, gp = ln[o:o + m].astype(np.int64), ptr[o:o + m].astype(np.int64)
        wl = want[i][1].astype(np.int64)
        assert np.array_equal(gl, wl), "pattern %d (%d bases) at (%d, %d): lengths differ first at %d" % (i, m, seg_len, overlap, int(np.nonzero(gl != wl)[0][0]))
        # Where the reference's own pointer is no text position - its walk went on matching after a byte the BWT does not hold, and 0 minus the
        # number of those matches is what its unsigned arithmetic leaves (moni.hpp:583-594) - the byte has reset the walk, so every walk gives the
        # same value: equal to the oracle's.  Everywhere else: pointer < n, and text[p : p + l] == pattern[k : k + l], compared directly wherever
        # it does not follow from k - 1 (the pointer one further, the length one less).
        odd = want[i][0] >= np.uint64(n)
        assert np.array_equal(ptr[o:o + m][odd], want[i][0][odd])
        assert not (ptr[o:o + m][~odd] >= np.uint64(n)).any()
        for k in np.nonzero(~odd)[0].tolist():
            l, q = int(gl[k]), int(gp[k])
            if k and not odd[k - 1] and q == int(gp[k - 1]) + 1 and l == int(gl[k - 1]) - 1:
                continue
            assert text[q:q + l] == p[k:k + l] and q + l <= len(text), "pattern %d offset %d: the text at %d does not hold %d bases of the pattern" % (i, k, q, l)
    assert st["segments"] == len(tab)
    assert st["steps_spec"] == steps_spec
    assert st["flagged"] == sum(flags) and st["chain_runs"] == runs
    assert st["steps_chain"] == steps_chain
    if all(len(p) <= seg_len for p in pats):          # nothing was cut: the walk is the reference's, pointers included
        for i, p in enumerate(pats):
            o = int(offs[i])
            assert np.array_equal(ptr[o:o + len(p)], want[i][0])
    return st, (tab, flags, runs), want


def mutate(seq: np.ndarray, rng, every=300, n_indels=4):
    """a haplotype with a substitution every ~`every` bases and a few indels"""
    s = seq.copy()
    at = int(rng.integers(every // 2, every))
    while at < len(s):
        s[at] = ACGT[(int(np.nonzero(ACGT == s[at])[0][0]) + int(rng.integers(1, 4))) % 4] if s[at] in ACGT else ACGT[0]
        at += int(rng.integers(every // 2, every + every // 2))
    for _ in range(n_indels):
        p = int(rng.integers(100, len(s) - 100))
        if rng.integers(0, 2):
            s = np.delete(s, slice(p, p + int(rng.integers(1, 4))))
        else:
            s = np.insert(s, p, ACGT[rng.integers(0, 4, size=int(rng.integers(1, 4)))])
    return s


def edge_lengths(seg_len):
    return [0, 1, 7, 8, 9, seg_len - 1, seg_len, seg_len + 1, 3 * seg_len + 5]


def ragged_batch(case, seg_len, overlap, seed=5):
    """(c) and (d) in one batch: the edge lengths on a mutated haplotype, one pattern of about 20 000 bases, and patterns with N, lower-case letters
    and a byte the BWT does not hold at a segment's first base, at its last base and inside an overlap region.  The odd lengths make the offsets
    ragged: groups of 8 output places straddle patterns."""
    rng = np.random.default_rng(seed)
    hap = mutate(case.pg.seqs[1], rng)
    pats, at = [], 37
    for L in edge_lengths(seg_len):
        pats.append(hap[at:at + L].tobytes())
        at += L + 11
    pats.append(mutate(case.pg.seqs[2][3000:23003], rng).tobytes())          # about 20 000 bases
    g0 = sum(len(p) for p in pats)
    m = max(6 * seg_len + 3, 600)
    base = mutate(case.pg.seqs[3][1000:1000 + m + 50], rng, every=10 ** 9, n_indels=0)[:m]
    for fill in (b"N", None, b"\x01"):
        p = bytearray(base.tobytes())
        cs = cuts(g0, m, seg_len, overlap)
        a, b, e = cs[len(cs) // 2]
        for k in {a, b - 1, min(b + overlap // 2, m - 1), cs[1][0] if len(cs) > 1 else 0, cs[0][1] - 1}:
            p[k:k + 1] = fill if fill else bytes(p[k:k + 1]).lower()
        pats.append(bytes(p))
        g0 += m
    # an absent byte right behind the first base of every segment: where the step before it happens to be a match, the reference's pointer at the
    # segment's first base is no text position, and its length is the one carried over from the segment on the left (odd_starts counts them)
    p = bytearray(base.tobytes())
    for a, b, e in cuts(g0, m, seg_len, overlap)[1:]:
        if b - a > 2:
            p[a + 1:a + 2] = b"N"
    pats.append(bytes(p))
    pats.append(bytes(base.tobytes()).lower()[:max(seg_len + 3, 40)])           # lower case throughout: every length 0
    return pats


def odd_starts(pats, want, n, seg_len, overlap):
    """segments (not the first of their pattern) whose first base has a reference pointer that is no text position"""
    return sum(1 for i, a, b, e in table(pats, seg_len, overlap) if a > 0 and int(want[i][0][a]) >= n)


def random_batch(seed=9):
    """(a) uniformly random ACGT: short matches"""
    rng = np.random.default_rng(seed)
    return [ACGT[rng.integers(0, 4, size=L)].tobytes() for L in (20000, 4097, 333)]


def substring_pattern(case, seg_len):
    """(b) a verbatim substring of the text of >= 10 segments; the last one is longer than any overlap of SETTINGS, so it alone has e == m"""
    L = 10 * seg_len + seg_len // 2 + 2
    return case.text[1234:1234 + L]


def haplotype_pattern(case, seed=13):
    """(c) a whole haplotype of the pangenome with a substitution every ~300 bases and a few indels"""
    return mutate(case.pg.seqs[4], np.random.default_rng(seed)).tobytes()
