"""SPUMONI's pseudo-matching lengths in plain Python: a restatement of ms_pointers<..., thr_bv<>>::_query (include/ms/spumoni.hpp:356-410) over a
flat index's F, heads, starts and thr, and the text of `moni pseudo-ms` (src/spumoni/run_spumoni.cpp:466-501).  The yardstick of the PML tests."""
from bisect import bisect_left, bisect_right

import numpy as np


class PmlModel:
    def __init__(self, fi):
        self.n, self.r = int(fi.n), int(fi.r)
        self.F = [int(x) for x in fi.F]
        heads = np.asarray(fi.heads)
        starts = np.asarray(fi.starts).astype(np.int64)
        lens = np.diff(starts)
        self.heads, self.starts = heads.tolist(), starts.tolist()          # plain lists: bisect on them is the searchsorted of this model
        self.n_c = [0] * 256
        self.runs, self.before, self.thr = {}, {}, {}          # per letter: its runs, the letters in front of each (one past the end too), their thresholds
        for c in np.unique(heads):
            k = np.nonzero(heads == c)[0]
            self.runs[int(c)] = k.tolist()
            self.before[int(c)] = np.concatenate(([0], np.cumsum(lens[k]))).tolist()
            self.thr[int(c)] = np.asarray(fi.thr)[k].tolist()
            self.n_c[int(c)] = int(lens[k].sum())

    def run_of_position(self, pos):
        """rle_string::run_of_position; position n lies in "run" r"""
        return bisect_right(self.starts, pos) - 1

    def walk(self, pattern: bytes):
        """(lengths, jumps): the pseudo-matching length at every read offset and the number of threshold jumps of the walk"""
        m = len(pattern)
        lengths = [0] * m
        pos, length, jumps = self.n - 1, 0, 0
        for i in range(m):
            c = pattern[m - i - 1]
            if self.n_c[c] == 0:                                   # spumoni.hpp:372-377: LF(pos, c) of a letter that does not occur = F[c]
                length = 0
                pos = self.F[c]
            else:
                run = self.run_of_position(pos)
                ck, before = self.runs[c], self.before[c]
                if pos < self.n and self.heads[run] == c:     # 378-383
                    length += 1
                    j = bisect_left(ck, run)              # run is the j-th run of c
                    pos = self.F[c] + before[j] + (pos - self.starts[run])
                else:                                              # 384-404
                    jumps += 1
                    j = bisect_left(ck, run)              # run_and_head_rank: j runs of c before `run`, before[j] letters c in them
                    if j == len(ck):
                        up = True                                  # no next run of c
                    elif j == 0:
                        up = False                                 # no previous one
                    else:
                        up = pos < self.thr[c][j]             # rnk_c.first > thresholds.rank(pos + 1, c)
                    pos = self.F[c] + before[j] - (1 if up else 0)
                    length = 0
            lengths[m - i - 1] = length
        return lengths, jumps

    def query(self, pattern: bytes):
        return self.walk(pattern)[0]

    def batch(self, reads, thr=25):
        """(lengths concatenated, read_max, read_hits) of a list of reads, as moni_pml_batch lays them out"""
        ls = [self.query(r) for r in reads]
        flat = np.array([x for l in ls for x in l], dtype=np.uint32)
        mx = np.array([max(l) if l else 0 for l in ls], dtype=np.uint32)
        hits = np.array([sum(1 for x in l if x >= thr) for l in ls], dtype=np.uint32)
        return flat, mx, hits


def render(lengths_per_read, first=0) -> bytes:
    """<out>.pseudo_lengths: per read ">" + its running number, then the lengths, each followed by a blank (run_spumoni.cpp:495-498)"""
    out = []
    for i, l in enumerate(lengths_per_read):
        out.append(b">%d\n" % (first + i))
        out.append(b"".join(b"%d " % int(x) for x in l) + b"\n")
    return b"".join(out)


def sim_reads(case, n=20, seed=31):
    """n simulated 150-base reads (2 % substitutions, a few indels) and the special ones: NNN inside, lower case, mixed case, length 1, empty"""
    reads = [r.tobytes() for r in case.synth.make_reads(case.pg, n, 150, seed=seed, sub_rate=0.02, indel_rate=0.003)]
    text = case.text
    reads.append(text[300:370] + b"NNN" + text[373:450])
    reads.append(text[500:650].lower())
    reads.append(mixed_case(text[900:1050]))
    reads.append(text[777:778])
    reads.append(b"")
    return reads


def mixed_case(r: bytes) -> bytes:
    """lower-case letters sort above every letter of the BWT, so the walk stands at position n ("run" r) after one and the next upper-case
    letter starts there: single ones, a pair, one at either end of the read"""
    b = bytearray(r)
    for k in (0, 40, 41, 90, len(b) - 1):
        b[k] = ord(chr(b[k]).lower())
    return bytes(b)


def ragged(reads):
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer(b"".join(reads), dtype=np.uint8).copy(), offs
