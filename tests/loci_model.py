"""Reference loci in plain Python over a flat index's arrays: LocateModel's backward search, seqcount_model's segments, phi inside each, and
liftidx::lift of every occurrence computed from the flat index's ins / del column lists (levioSAM's lift_pos = ins.rank0(del.select0(p + 1))); the
keys folded per task.  The yardstick of the host replay (tests/test_host_loci.py); tests/test_loci_model.py checks it against brute force."""
from collections import Counter

import numpy as np

from tests import locate_model as lm
from tests import seqcount_model as sm

RES_DTYPE = np.dtype([("count", "<u8"), ("sa_lo", "<u8"), ("loci_off", "<u8"), ("n_loci", "<u8"), ("matched", "<u4"), ("walked", "<u4"), ("n_segs", "<u4"),
                      ("reserved", "<u4")])


class LociModel(sm.SeqcountModel):
    def __init__(self, fi):
        super().__init__(fi)
        self.lifts = []                                  # per sequence (second, column of every haplotype position, reference bases in front of every column, columns, reference bases)
        lf = getattr(fi, "lifts", None)
        for i in range(len(self.seq_starts) - 1):
            if lf is None:
                self.lifts.append(None)
                continue
            cols = int(lf.len[i])
            ins, dele = np.zeros(cols, bool), np.zeros(cols, bool)
            ins[lf.ins_of(i).astype(np.int64)] = True
            dele[lf.del_of(i).astype(np.int64)] = True
            ref_before = np.cumsum(~ins) - (~ins)
            self.lifts.append((int(lf.second[i]), np.nonzero(~dele)[0], ref_before, cols, int((~ins).sum())))

    def lift(self, p):
        """liftidx::lift(p): the sequence of p, then second + lift_pos(offset inside it); past the lift's columns (the separator bytes) positions go
        on one to one"""
        sid = int(self.seq_of(p))
        L = self.lifts[sid]
        if L is None:
            return p
        second, hap_cols, ref_before, cols, n_ref = L
        ph = p - int(self.seq_starts[sid])
        if ph < len(hap_cols):
            return second + int(ref_before[hap_cols[ph]])
        return second + n_ref + (ph - len(hap_cols))

    def task(self, pattern: bytes, lift=1, max_walk=1 << 20):
        """(count, sa_lo, matched, walked, n_segs), [(key, support)] ascending, phi steps"""
        count, sa_lo, matched, toe = self.search(pattern)
        walked = int(max_walk == 0 or count <= max_walk)
        segs = self.segments(sa_lo, count, toe) if walked and count else []
        keys, phi = Counter(), 0
        for t, ln in segs:
            phi += ln - 1
            for p in self.locate(t, ln):
                keys[self.lift(p) if lift else p] += 1
        return (count, sa_lo, matched, walked, len(segs)), sorted(keys.items()), phi

    def loci_batch(self, patterns, strands=1, lift=1, max_walk=1 << 20):
        """(res, lpos, lseq, lseq_off, support, phi steps) as moni_loci_batch lays them out: task i * strands + s"""
        res = np.zeros(len(patterns) * strands, dtype=RES_DTYPE)
        lpos, sup, phi = [], [], 0
        for i, p in enumerate(patterns):
            for s in range(strands):
                (count, sa_lo, matched, walked, n_segs), loci, k = self.task(lm.revcomp(p) if s else p, lift, max_walk)
                res[i * strands + s] = (count, sa_lo, len(lpos), len(loci), matched, walked, n_segs, 0)
                lpos += [a for a, _ in loci]
                sup += [b for _, b in loci]
                phi += k
        lpos = np.array(lpos, dtype=np.uint64)
        sq = self.seq_of(lpos).astype(np.uint32) if len(lpos) else np.zeros(0, np.uint32)
        so = (lpos.astype(np.int64) - self.seq_starts[sq]).astype(np.uint64) if len(lpos) else np.zeros(0, np.uint64)
        return res, lpos, sq, so, np.array(sup, dtype=np.uint64), phi


# ---- brute force: nothing shared with the model or the library but the text (and, for the lift, the pangenome's variant lists) -------------

def hap_to_ref(pg, h):
    """for every base of haplotype h (sequence h + 1) the reference base it lifts to: a SNP stays, the bases of an insertion before reference base p
    all go to p, a deletion of [p, p + len) is skipped"""
    pos, kind, ln = pg.variants[h]
    out, prev = [], 0
    for p, k, l in zip(pos.tolist(), kind.tolist(), ln.tolist()):
        out.extend(range(prev, p))
        if k == 0:
            out.append(p)
            prev = p + 1
        elif k == 1:
            out.extend([p] * l)
            prev = p
        else:
            prev = p + l
    out.extend(range(prev, len(pg.seqs[0])))
    assert len(out) == len(pg.seqs[h + 1])
    return out


def text_to_ref(pg):
    """text position -> lifted position for a pangenome whose haplotypes lift onto sequence 0 (which starts at text position 0); -1 in the separators"""
    out = []
    for i, s in enumerate(pg.seqs):
        out += (list(range(len(s))) if i == 0 else hap_to_ref(pg, i - 1)) + [-1] * pg.w
    out += [-1] * (pg.w - 1)
    return np.array(out, dtype=np.int64)


def brute_loci(text: bytes, q: bytes, keymap=None):
    """(count, matched, [(key, support)] ascending): all start positions of q by direct search, mapped through keymap (None: the position itself)"""
    count, matched, _ = lm.brute(text, q)
    occ = lm.occurrences(text, q)
    keys = occ if keymap is None else [int(keymap[i]) for i in occ]
    assert all(k >= 0 for k in keys)                     # no occurrence starts in a separator
    return count, matched, sorted(Counter(keys).items())


def check_against_brute(text: bytes, patterns, out, strands, max_walk, seq_starts, keymap=None):
    """out = (res, lpos, lseq, lseq_off, support) in the library's layout against brute force, value for value (sa_lo is left to the model and to
    locate's tests); returns the number of loci"""
    res, lpos, lseq, lseq_off, support = out[:5]
    seq_starts = np.asarray(seq_starts).astype(np.int64)
    assert len(res) == len(patterns) * strands
    at = 0
    for i, p in enumerate(patterns):
        for s in range(strands):
            q = lm.revcomp(p) if s else p
            count, matched, loci = brute_loci(text, q, keymap)
            r = res[i * strands + s]
            walked = int(max_walk == 0 or count <= max_walk)
            assert (int(r["count"]), int(r["matched"]), int(r["walked"])) == (count, matched, walked), (i, s, q[:40], r, count, matched)
            if not walked:
                assert int(r["n_loci"]) == 0 and int(r["n_segs"]) == 0
                continue
            assert int(r["n_loci"]) == len(loci) and (int(r["n_segs"]) > 0) == (count > 0), (i, s, q[:40], r, len(loci))
            if loci:
                assert int(r["loci_off"]) == at, (i, s)
                k = len(loci)
                assert [int(x) for x in lpos[at:at + k]] == [a for a, _ in loci], (i, s, q[:40])
                assert [int(x) for x in support[at:at + k]] == [b for _, b in loci], (i, s, q[:40])
                assert int(support[at:at + k].sum()) == count
                want_sq = np.minimum(np.searchsorted(seq_starts, lpos[at:at + k].astype(np.int64), side="right") - 1, len(seq_starts) - 2)
                assert np.array_equal(lseq[at:at + k], want_sq) and np.array_equal(lseq_off[at:at + k].astype(np.int64), lpos[at:at + k].astype(np.int64) - seq_starts[want_sq])
                at += k
    assert at == len(lpos) == len(lseq) == len(lseq_off) == len(support)
    return at


# ---- the shared lifted case: six sequences of about 6 k bases, the haplotypes with SNPs, insertions and deletions against the first ----------------

_case = {}


def lifted_case(lifted=True):
    """(pangenome, flat index, text, patterns): synth.make_pangenome(6000, 5, site_spacing=120), with its lifts or (lifted=False) as the FASTA-built
    form of the same text.  The patterns are upper-case ACGT only: none starts in a separator."""
    if lifted not in _case:
        from moni_align_amd import index_build, synth
        pg = synth.make_pangenome(6000, 5, site_spacing=120)
        fi = index_build.build_from_pangenome(pg, device="cpu", lifted=lifted)
        text = fi.text.tobytes()
        ref = pg.seqs[0].tobytes()
        h1 = pg.seqs[1].tobytes()
        ins = inside_insertion(pg)
        hd, dl = behind_deletion(pg)
        pats = [b"A", b"ACG", ref[1000:1032], h1[ins:ins + 20], ref[2784:2804], b"C", b"GT", b"ACGTAC", ref[5:45], b"TTTTTTTTTTTTTTTT", b""]
        pats.append(pg.seqs[hd + 1].tobytes()[dl:dl + 20])          # a 20-mer whose first base is the one just behind a deletion
        pats += [ref[a:a + 24] for a in range(200, 5800, 400)] + [h1[a:a + 18] for a in range(150, 5800, 700)]
        _case[lifted] = (pg, fi, text, pats)
    return _case[lifted]


def inside_insertion(pg):
    """a position of haplotype 1 (sequence 1) inside its 4-base insertion in front of reference base 2784"""
    pos, kind, ln = pg.variants[0]
    m = hap_to_ref(pg, 0)
    k = [j for j, (p, kd, l) in enumerate(zip(pos.tolist(), kind.tolist(), ln.tolist())) if kd == 1 and p == 2784 and l == 4]
    assert k, "the pangenome has no 4-base insertion before reference base 2784 in haplotype 1"
    return m.index(2784) + 1                             # the second of the four inserted bases


def behind_deletion(pg):
    """(haplotype, position in it) of the first base that follows a deletion"""
    for h in range(len(pg.variants)):
        m = hap_to_ref(pg, h)
        for j in range(1, len(m)):
            if m[j] - m[j - 1] > 1:
                return h, j
    raise AssertionError("the pangenome has no deletion")
