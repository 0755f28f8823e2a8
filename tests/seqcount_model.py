"""Per-sequence occurrence counts in plain Python over a flat index's arrays: LocateModel's backward search, then the interval cut at the BWT run
boundaries - one segment per run, its toehold the run's last suffix-array sample (the task's own toehold for the run of the upper end) - and phi
downwards inside each segment.  The yardstick of the host replay (tests/test_host_seqcount.py); tests/test_seqcount_model.py checks it against
brute force."""
import numpy as np

from tests import locate_model as lm

RES_DTYPE = np.dtype([("count", "<u8"), ("sa_lo", "<u8"), ("matched", "<u4"), ("n_seqs", "<u4"), ("walked", "<u4"), ("n_segs", "<u4")])


class SeqcountModel(lm.LocateModel):
    def segments(self, sa_lo, count, toe):
        """[(toehold, length)] of the interval [sa_lo, sa_lo + count - 1], in run order"""
        hi = sa_lo + count - 1
        k_lo, k_hi = self.run_of_position(sa_lo), self.run_of_position(hi)
        out = []
        for k in range(k_lo, k_hi + 1):
            a = max(sa_lo, self.starts[k])
            if k == k_hi:
                out.append((toe, hi - a + 1))
            else:
                out.append(((self.esa[k] + 1) % self.n, self.starts[k + 1] - a))
        return out

    def task(self, pattern: bytes, max_walk=1 << 20):
        """(record, row, phi steps)"""
        n_seq = len(self.seq_starts) - 1
        count, sa_lo, matched, toe = self.search(pattern)
        row = np.zeros(n_seq, dtype=np.uint64)
        walked = int(max_walk == 0 or count <= max_walk)
        segs = self.segments(sa_lo, count, toe) if walked and count else []
        phi = 0
        for t, ln in segs:
            pos = self.locate(t, ln)
            phi += ln - 1
            np.add.at(row, self.seq_of(pos), 1)
        return (count, sa_lo, matched, int((row != 0).sum()), walked, len(segs)), row, phi

    def seq_batch(self, patterns, strands=1, max_walk=1 << 20):
        """(res, counts, phi steps) as moni_seqcount_batch lays them out: task i * strands + s"""
        n_seq = len(self.seq_starts) - 1
        res = np.zeros(len(patterns) * strands, dtype=RES_DTYPE)
        counts = np.zeros((len(res), n_seq), dtype=np.uint64)
        phi = 0
        for i, p in enumerate(patterns):
            for s in range(strands):
                rec, row, k = self.task(lm.revcomp(p) if s else p, max_walk)
                res[i * strands + s] = rec
                counts[i * strands + s] = row
                phi += k
        return res, counts, phi


# ---- brute force: nothing shared with the model or the library but the text and the sequence starts -----------------------------------

def brute_row(text: bytes, q: bytes, seq_starts):
    """(count, matched, row): all start positions of q by direct search, binned with numpy.searchsorted on the sequence starts"""
    seq_starts = np.asarray(seq_starts).astype(np.int64)
    n_seq = len(seq_starts) - 1
    m, matched = len(q), 0
    while matched < m and text.find(q[m - 1 - matched:]) >= 0:
        matched += 1
    occ, i = [], text.find(q) if q else -1
    while i >= 0:
        occ.append(i)
        i = text.find(q, i + 1)
    sid = np.minimum(np.searchsorted(seq_starts, np.array(occ, dtype=np.int64), side="right") - 1, n_seq - 1)
    return len(occ), matched, np.bincount(sid, minlength=n_seq).astype(np.uint64)


def check_against_brute(text: bytes, patterns, res, counts, strands, max_walk, seq_starts):
    """res / counts in the library's layout against brute force, value for value (sa_lo is left to the model and to locate's tests)"""
    n_seq = len(seq_starts) - 1
    assert len(res) == len(patterns) * strands and counts.shape == (len(res), n_seq)
    for i, p in enumerate(patterns):
        for s in range(strands):
            q = lm.revcomp(p) if s else p
            count, matched, row = brute_row(text, q, seq_starts)
            r, t = res[i * strands + s], i * strands + s
            walked = int(max_walk == 0 or count <= max_walk)
            assert (int(r["count"]), int(r["matched"]), int(r["walked"])) == (count, matched, walked), (i, s, q[:40], r, count, matched)
            if walked:
                assert np.array_equal(counts[t], row), (i, s, q[:40], counts[t], row)
                assert int(counts[t].sum()) == count and int(r["n_seqs"]) == int((row != 0).sum())
                assert (int(r["n_segs"]) > 0) == (count > 0) and int(r["n_segs"]) <= max(count, 0)
            else:
                assert not counts[t].any() and int(r["n_seqs"]) == 0 and int(r["n_segs"]) == 0
