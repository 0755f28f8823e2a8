"""Depth of coverage as DESIGN.md 7.17 defines it, in plain Python over the standard library, numpy's arrays and tests/bam_model's header reader.
No project code, and written from the definition, not from the kernels.

References r of lengths LN_r (the header's @SQ lines).  A record counts iff refID >= 0, pos >= 0, n_cigar_op > 0, flag & exclude == 0 and
mapq >= min_mapq; a record that fails several of these is unplaced before skipped_flag before skipped_mapq.  Its CIGAR is walked from pos:
M = X D cover and advance, N advances without covering, I S H P do nothing; covering operations with no N between them are one block, and
a block without a base is none.  A block is clipped to LN_r, dropped when it begins at or behind LN_r (the record is `clipped`, once), and
otherwise adds one to the depth of every base it covers.  No mate-overlap correction."""
import struct

import numpy as np

from tests import bam_model as bam
from tests import bamsort_model as bsm

EXCLUDE, MIN_MAPQ = 0x704, 0
LIMIT = 1 << 31


def blocks(rec: bytes):
    """[(begin, end)] of one record's CIGAR on its reference, unclipped"""
    pos, l_name, n_ops = struct.unpack_from("<i", rec, 8)[0], rec[12], struct.unpack_from("<H", rec, 16)[0]
    out, p, start = [], pos, pos
    for k in range(n_ops):
        v = struct.unpack_from("<I", rec, 36 + l_name + 4 * k)[0]
        op = bam.OPS[v & 15] if v & 15 < len(bam.OPS) else "?"
        if op in "M=XD":
            p += v >> 4
        elif op == "N":
            if p > start:
                out.append((start, p))
            p += v >> 4
            start = p
    if p > start:
        out.append((start, p))
    return out


def classify(rec: bytes, exclude: int = EXCLUDE, min_mapq: int = MIN_MAPQ) -> str:
    ref, pos, _, mapq, _, n_ops, flag = struct.unpack_from("<iiBBHHH", rec, 4)
    if ref < 0 or pos < 0 or n_ops == 0:
        return "unplaced"
    if flag & exclude:
        return "skipped_flag"
    if mapq < min_mapq:
        return "skipped_mapq"
    return "counted"


class Coverage:
    """the depth of every reference of `header` under the records given to add()"""

    def __init__(self, header: bytes, exclude: int = EXCLUDE, min_mapq: int = MIN_MAPQ):
        self.refs = bam.references(header)
        self.exclude, self.min_mapq = exclude, min_mapq
        self.diff = [np.zeros(ln + 1, np.int64) for _, ln in self.refs]
        self.stats = dict(records=0, counted=0, skipped_flag=0, skipped_mapq=0, unplaced=0, clipped=0, blocks=0)

    def add(self, recs):
        for rec in recs:
            self.stats["records"] += 1
            c = classify(rec, self.exclude, self.min_mapq)
            self.stats[c] += 1
            if c != "counted":
                continue
            ref = struct.unpack_from("<i", rec, 4)[0]
            ln, clipped = self.refs[ref][1], False
            for b, e in blocks(rec):
                if b >= ln:
                    clipped = True
                    continue
                if e > ln:
                    e, clipped = ln, True
                self.diff[ref][b] += 1
                self.diff[ref][e] -= 1
                self.stats["blocks"] += 1
            self.stats["clipped"] += clipped
        return self

    def depth(self, r: int) -> np.ndarray:
        """the depth of every base of reference r"""
        return np.cumsum(self.diff[r])[:-1]

    def per_base(self) -> bytes:
        """mosdepth's per-base.bed: the maximal runs of equal depth of every reference, zero included"""
        out = []
        for r, (name, ln) in enumerate(self.refs):
            d = self.depth(r)
            cuts = np.concatenate([[0], np.flatnonzero(d[1:] != d[:-1]) + 1, [ln]])
            out.extend(b"%s\t%d\t%d\t%d\n" % (name, a, b, d[a]) for a, b in zip(cuts[:-1].tolist(), cuts[1:].tolist()))
        return b"".join(out)

    def ref_figures(self):
        """[(length, bases, min, max)] per reference"""
        return [(ln, int(self.depth(r).sum()), int(self.depth(r).min()), int(self.depth(r).max())) for r, (_, ln) in enumerate(self.refs)]

    def summary(self) -> bytes:
        return summary_text([n for n, _ in self.refs], self.ref_figures())

    def windows(self, r: int, window: int):
        d = self.depth(r)
        return [int(d[a:a + window].sum()) for a in range(0, len(d), window)]

    def regions(self, window: int) -> bytes:
        """chrom, start, end, the mean depth of the window to two places"""
        out = []
        for r, (name, ln) in enumerate(self.refs):
            for k, s in enumerate(self.windows(r, window)):
                a, b = k * window, min((k + 1) * window, ln)
                out.append(b"%s\t%d\t%d\t%s\n" % (name, a, b, b"%.2f" % (s / (b - a))))
        return b"".join(out)

    def mean_depth(self) -> float:
        f = self.ref_figures()
        length = sum(x[0] for x in f)
        return sum(x[1] for x in f) / length if length else 0.0


def summary_text(names, figures) -> bytes:
    """mosdepth's summary.txt from [(length, bases, min, max)]: a row per reference, then the total"""
    out = [b"chrom\tlength\tbases\tmean\tmin\tmax\n"]
    rows = [(n,) + tuple(f) for n, f in zip(names, figures)]
    if rows:
        rows.append((b"total", sum(r[1] for r in rows), sum(r[2] for r in rows), min(r[3] for r in rows), max(r[4] for r in rows)))
    else:
        rows.append((b"total", 0, 0, 0, 0))
    for name, length, bases, mn, mx in rows:
        out.append(b"%s\t%d\t%d\t%s\t%d\t%d\n" % (name, length, bases, b"%.2f" % (bases / length if length else 0.0), mn, mx))
    return b"".join(out)


def of_bam_file(data: bytes, exclude: int = EXCLUDE, min_mapq: int = MIN_MAPQ) -> Coverage:
    """the model over the records of a BAM file's bytes"""
    f = bsm.BamFile(data)
    return Coverage(f.text, exclude, min_mapq).add(f.recs)
