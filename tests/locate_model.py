"""Exact-match count and locate in plain Python: the backward search of an r-index (ri::r_index::count / locate_all, which the reference's
ms_pointers inherits) over a flat index's F, heads, starts, ssa and esa, with the toehold bookkeeping of ms_pointers::_query
(include/ms/moni.hpp:568-624).  The yardstick of the host replay; tests/test_locate_model.py checks it against brute force."""
from bisect import bisect_left, bisect_right

import numpy as np

RES_DTYPE = np.dtype([("count", "<u8"), ("sa_lo", "<u8"), ("occ_off", "<u8"), ("n_occ", "<u4"), ("matched", "<u4")])

_COMPL = bytearray(range(256))          # the aligner's table (include/common/kpbseq.h:120-137): lower case complements to upper case
for _a, _b in zip(b"ACGTacgt", b"TGCATGCA"):
    _COMPL[_a] = _b
COMPL = bytes(_COMPL)


def revcomp(p: bytes) -> bytes:
    return p.translate(COMPL)[::-1]


class LocateModel:
    def __init__(self, fi):
        self.n, self.r = int(fi.n), int(fi.r)
        self.F = [int(x) for x in fi.F]
        heads = np.asarray(fi.heads)
        starts = np.asarray(fi.starts).astype(np.int64)
        lens = np.diff(starts)
        self.heads, self.starts = heads.tolist(), starts.tolist()
        self.ssa, self.esa = [int(x) for x in fi.ssa], [int(x) for x in fi.esa]
        self.seq_starts = np.asarray(fi.seq_starts).astype(np.int64)
        self.runs, self.before = {}, {}          # per letter: its runs, and the letters in front of each of them (one past the last too)
        for c in np.unique(heads):
            k = np.nonzero(heads == c)[0]
            self.runs[int(c)] = k.tolist()
            self.before[int(c)] = np.concatenate(([0], np.cumsum(lens[k]))).tolist()
        # phi: SA[first position of run k] = ssa[k] + 1 and SA[last position of run k - 1] = esa[k - 1] + 1 (both mod n)
        self.phi_keys = sorted(((self.ssa[k] + 1) % self.n, k) for k in range(self.r))

    def run_of_position(self, pos):
        return bisect_right(self.starts, pos) - 1

    def search(self, pattern: bytes):
        """(count, sa_lo, matched, toehold): the interval's size and first BWT position, the bytes consumed while it held a position, SA[upper end]"""
        m = len(pattern)
        lo, hi = 0, self.n - 1
        toe = (self.esa[self.r - 1] + 1) % self.n
        matched = 0
        for i in range(m):
            c = pattern[m - 1 - i]
            if c <= 1 or c not in self.runs:
                return 0, 0, matched, 0
            ck, before = self.runs[c], self.before[c]
            run = self.run_of_position(lo)
            j = bisect_left(ck, run)                         # runs of c in front of `run`
            nlo = self.F[c] + before[j] + (lo - self.starts[run] if self.heads[run] == c else 0)
            run = self.run_of_position(hi)
            j = bisect_left(ck, run)
            if self.heads[run] == c:
                nhi = self.F[c] + before[j] + (hi - self.starts[run])
                ntoe = toe - 1
            else:                                            # one before the image of the next c-run's first position: the last c above
                nhi = self.F[c] + before[j] - 1
                ntoe = self.esa[ck[j - 1]] if j else 0
            if nlo > nhi:
                return 0, 0, matched, 0
            lo, hi, toe = nlo, nhi, ntoe
            matched += 1
        if m == 0:
            return 0, 0, 0, 0
        return hi - lo + 1, lo, matched, toe

    def phi(self, i):
        """SA[rank - 1] of the suffix i = SA[rank]"""
        k = bisect_right(self.phi_keys, (i, self.r)) - 1     # the last run start whose suffix lies at or in front of i (circular)
        key, run = self.phi_keys[k]
        return (self.esa[run - 1] + 1 + (i - key) % self.n) % self.n

    def locate(self, toe, n_occ):
        out, p = [], toe
        for k in range(n_occ):
            if k:
                p = self.phi(p)
            out.append(p)
        return out

    def seq_of(self, pos):
        s = np.searchsorted(self.seq_starts, np.asarray(pos, dtype=np.int64), side="right") - 1
        return np.minimum(s, len(self.seq_starts) - 2)

    def batch(self, patterns, strands=1, max_occ=0):
        """(res, pos, seq, seq_off) as moni_locate_batch lays them out: task i * strands + s"""
        res = np.zeros(len(patterns) * strands, dtype=RES_DTYPE)
        pos = []
        for i, p in enumerate(patterns):
            for s in range(strands):
                count, sa_lo, matched, toe = self.search(revcomp(p) if s else p)
                k = min(count, max_occ)
                res[i * strands + s] = (count, sa_lo, len(pos) if max_occ else 0, k, matched)
                pos += self.locate(toe, k)
        pos = np.array(pos, dtype=np.uint64)
        sq = self.seq_of(pos).astype(np.uint32) if len(pos) else np.zeros(0, np.uint32)
        so = (pos.astype(np.int64) - self.seq_starts[sq]).astype(np.uint64) if len(pos) else np.zeros(0, np.uint64)
        return res, pos, sq, so


# ---- brute force: nothing shared with the model or the library but the text ----------------------------------------------------------

def occurrences(text: bytes, p: bytes):
    """every i with text[i:i+m] == p, increasing"""
    out, i = [], text.find(p) if p else -1
    while i >= 0:
        out.append(i)
        i = text.find(p, i + 1)
    return out


def by_rank(text: bytes, occ, limit=None):
    """positions ordered as their suffixes are in the suffix array of text + terminator (the terminator is the smallest byte: a suffix that is a
    prefix of another one sorts first, as bytes objects compare).  limit: compare that many bytes of a suffix only (a long text with many
    occurrences) - exact where the prefixes are pairwise distinct, which is asserted"""
    if limit is None:
        return sorted(occ, key=lambda i: text[i:])
    keys = {i: text[i:i + limit] for i in occ}
    assert len(set(keys.values())) == len(keys)
    return sorted(occ, key=keys.get)


def brute(text: bytes, p: bytes, max_occ=0, limit=None):
    """(count, matched, kept): occurrences, the longest suffix of p that occurs, the max_occ highest ranks in decreasing rank order"""
    m = len(p)
    matched = 0
    while matched < m and text.find(p[m - 1 - matched:]) >= 0:
        matched += 1
    occ = occurrences(text, p)
    kept = by_rank(text, occ, limit)[::-1][:max_occ] if max_occ else []
    return len(occ), matched, kept


def naive_sa(text: bytes):
    return by_rank(text, range(len(text) + 1))


def ragged(patterns):
    offs = np.zeros(len(patterns) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in patterns])
    return np.frombuffer(b"".join(patterns), dtype=np.uint8).copy(), offs


def check_against_brute(text: bytes, patterns, res, pos, sq, so, strands, max_occ, seq_starts, rank_of=None, limit=None):
    """res / pos / sq / so in the library's layout against brute force, value for value; rank_of: inverse of the naive suffix array (sa_lo)"""
    assert len(res) == len(patterns) * strands
    seq_starts = np.asarray(seq_starts).astype(np.int64)
    at = 0
    for i, p in enumerate(patterns):
        for s in range(strands):
            q = revcomp(p) if s else p
            count, matched, kept = brute(text, q, max_occ, limit)
            r = res[i * strands + s]
            assert (int(r["count"]), int(r["matched"]), int(r["n_occ"])) == (count, matched, min(count, max_occ)), (i, s, q[:40], r, count, matched)
            if count and rank_of is not None:
                assert int(r["sa_lo"]) == min(rank_of[x] for x in occurrences(text, q)), (i, s)
            k = int(r["n_occ"])
            if k:
                assert int(r["occ_off"]) == at, (i, s)
                got = [int(x) for x in pos[at:at + k]]
                assert got == kept, (i, s, got, kept)
                for x in got:                                     # the self-check: the pattern stands there
                    assert text[x:x + len(q)] == q
                want_sq = np.minimum(np.searchsorted(seq_starts, np.array(got), side="right") - 1, len(seq_starts) - 2)
                assert np.array_equal(sq[at:at + k], want_sq) and np.array_equal(so[at:at + k].astype(np.int64), np.array(got) - seq_starts[want_sq])
                at += k
    assert at == len(pos) == len(sq) == len(so)


# ---- the shared small case: three sequences, about 4 k bases, planted repeats ------------------------------------------------------------

_case = None


def planted_case():
    """(flat index, text, patterns): a 3-sequence text with a 40-base unit planted nine times, a second sequence that is a mutated copy of part of
    the first, N runs (a fifth letter: no hot slot) and a poly-A stretch; the patterns cover the pattern-word and code-word edges, a whole
    sequence, patterns that die at the first, a middle and the last step, absent bytes, lower case, and N against N.  Built once."""
    global _case
    if _case is None:
        from moni_align_amd import index_build, synth
        rng = np.random.default_rng(2024)
        acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
        rnd = lambda k: acgt[rng.integers(0, 4, size=k)]
        unit = rnd(40)
        s0 = np.concatenate([rnd(300), unit, rnd(250), unit, rnd(100), np.frombuffer(b"A" * 30, np.uint8), rnd(200), unit, rnd(397)])
        s1 = s0[150:1250].copy()
        for k in range(40, len(s1), 97):
            s1[k] = acgt[(int(np.nonzero(acgt == s1[k])[0][0]) + 1) & 3]
        s1[500:504] = ord("N")
        s2 = np.concatenate([unit, rnd(333), unit, unit, rnd(301), np.frombuffer(b"NN", np.uint8), rnd(180), unit, rnd(255), unit])
        pg = synth.Pangenome(seqs=[s0, s1, s2], names=["ref", "hap1", "other"], w=10)
        fi = index_build.build_from_pangenome(pg, device="cpu")
        text = fi.text.tobytes()
        b0, b1, b2 = s0.tobytes(), s1.tobytes(), s2.tobytes()
        pats = [b0[700:700 + L] for L in (1, 2, 7, 8, 9, 31, 32, 33, 150)]
        pats += [b1[3:3 + L] for L in (1, 2, 7, 8, 9, 31, 32, 33, 150)]
        pats += [b1, unit.tobytes(), unit.tobytes()[5:30], b"A" * 12, b"A" * 30, b"A" * 31]
        pats += [b"", b"X", b0[100:140] + b"X", b0[100:120] + b"X" + b0[121:140], b"X" + b0[101:140]]          # an absent byte: last, middle, first
        broken = bytearray(b0[900:940]); broken[0] = ord("ACGT"["ACGT".index(chr(broken[0])) - 1])            # dies at the last step, if this 40-mer is absent
        pats.append(bytes(broken))
        broken = bytearray(b0[900:940]); broken[20] = ord("ACGT"["ACGT".index(chr(broken[20])) - 1])          # ... in the middle
        pats.append(bytes(broken))
        pats += [b0[400:450].lower(), b0[400:449] + b0[449:450].lower(), b"acgt"]                               # lower case never matches on strand 0
        pats += [b1[480:520], b"N", b"NN", b"NNNN", b"NNNNN", b1[499:501], b"ANA"]                                # N against the Ns of the text
        pats += [b"\x00", b"\x01", b0[10:20] + b"\x01", bytes([synth.SEP_SEQ]) * 3, b0[-5:] + bytes([synth.SEP_SEQ]) * 10 + b1[:5]]
        pats += [synth.revcomp(np.frombuffer(b2[50:110], np.uint8)[None, :])[0].tobytes(), synth.revcomp(unit[None, :])[0].tobytes()]
        _case = (fi, text, pats)
    return _case
