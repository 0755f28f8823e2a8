"""Duplicate marking as DESIGN.md 7.15 fixes it (Picard's rule without optical duplicates or UMIs), in plain Python over the standard library and
tests/bam_model / tests/bamsort_model's record readers.  No project code; written from the definitions, with dictionaries where the
library sorts.

  signature(rec, n_ref)        (takes part, end code e, score) of one raw record
  entries(recs, paired, n_ref) the entries of one run's records in input order: (k1, k2, score, kind, (i, j)), i and j indices into recs
  resolve(runs_entries)        {(run, index into the run's records)}: the duplicates
  mark(runs, paired, n_ref)    the two together; set_flags(recs, marked_indices) sets 0x400

Bad records raise MarkdupError(reason, index): the lowest index over all bad records, and of that record the first reason in the order
SEQ, CLIP, MATE.  A byte of 0xFF in QUAL counts 0 (it is no Phred value: BAM writes it for a missing QUAL); a score saturates at 2^31 - 1;
a record without a reference (refID -1) takes the id n_ref, as in the sort key.  In a paired run a record with flag & 1 must carry its
read's bit (0x40 for record 2p, 0x80 for 2p + 1) and not the other's; a record without flag & 1 is not asked - the aligner writes a pair it
could not align as two records of flag 4 -, and the two names are equal in every case."""
import struct

from tests import bam_model as bam
from tests import bamsort_model as bsm

SEQ, CLIP, MATE = 8, 9, 10
NONE = 0xFFFFFFFF


class MarkdupError(ValueError):
    def __init__(self, reason, index, count=None):
        self.reason, self.index, self.count = reason, index, count
        super().__init__("record %s: reason %d" % (index, reason))


def _head(rec):
    ref, pos, l_name, _, _, n_ops, flag, l_seq = struct.unpack_from("<iiBBHHHI", rec, 4)
    return ref, pos, l_name, n_ops, flag, l_seq


def signature(rec: bytes, n_ref: int):
    """(takes part, e, score); raises MarkdupError(SEQ or CLIP, None)"""
    ref, pos, l_name, n_ops, flag, l_seq = _head(rec)
    qual = 36 + l_name + 4 * n_ops + (l_seq + 1) // 2
    if len(rec) < qual + l_seq:
        raise MarkdupError(SEQ, None)
    if flag & 4 or flag & 0x900:
        return False, 0, 0
    ops = [struct.unpack_from("<I", rec, 36 + l_name + 4 * k)[0] for k in range(n_ops)]
    ops = [(v >> 4, bam.OPS[v & 15]) for v in ops]
    reflen = sum(n for n, c in ops if c in "MDN=X")
    lead = trail = 0
    a, b = 0, len(ops)
    while a < b and ops[a][1] in "SH":
        lead += ops[a][0]
        a += 1
    while b > a and ops[b - 1][1] in "SH":
        trail += ops[b - 1][0]
        b -= 1
    rev = flag >> 4 & 1
    u5 = pos + reflen - 1 + trail if rev else pos - lead
    if not -2 ** 31 <= u5 < 3 * 2 ** 31:
        raise MarkdupError(CLIP, None)
    e = ((n_ref if ref < 0 else ref) << 34 | (u5 + 2 ** 31) << 1 | rev) & (2 ** 64 - 1)
    score = sum(q for q in rec[qual:qual + l_seq] if 15 <= q != 0xFF)
    return True, e, min(score, 2 ** 31 - 1)


def _name(rec):
    return rec[36:36 + rec[12]]


def entries(recs, paired: bool, n_ref: int):
    """the entries of one run, in input order; raises MarkdupError with the lowest bad index and the number of bad records / units"""
    bad = []
    sigs = []
    for i, r in enumerate(recs):
        try:
            sigs.append(signature(r, n_ref))
        except MarkdupError as x:
            bad.append((i, x.reason))
            sigs.append((False, 0, 0))
    out = []
    if not paired:
        out = [(e, 0, s, 0, (i, None)) for i, (part, e, s) in enumerate(sigs) if part]
    else:
        for p in range((len(recs) + 1) // 2):
            i, j = 2 * p, 2 * p + 1
            if j >= len(recs):
                bad.append((i, MATE))
                continue
            f1, f2 = _head(recs[i])[4], _head(recs[j])[4]
            if (f1 & 1 and f1 & 0xC0 != 0x40) or (f2 & 1 and f2 & 0xC0 != 0x80) or _name(recs[i]) != _name(recs[j]):
                bad.append((i, MATE))
                continue
            (p1, e1, s1), (p2, e2, s2) = sigs[i], sigs[j]
            if p1 and p2 and f1 & 1 and f2 & 1:
                lo_is_read1 = e1 <= e2
                same_strand = (e1 & 1) == (e2 & 1)
                out.append((min(e1, e2), max(e1, e2), s1 + s2, 3 if same_strand and not lo_is_read1 else 1, (i, j)))
            else:
                out += [(e, 0, s, 0, (k, None)) for k, (part, e, s) in ((i, sigs[i]), (j, sigs[j])) if part]
    if bad:
        index, reason = min(bad)
        raise MarkdupError(reason, index, len(bad))
    return out


def resolve(runs_entries):
    """runs_entries[r]: entries of run r.  Returns {(r, i)} of the duplicates; input order is (run, place in the run's list)."""
    marked = set()
    pairs, ends = {}, {}
    for r, ents in enumerate(runs_entries):
        for k, (k1, k2, score, kind, (i, j)) in enumerate(ents):
            if kind:
                pairs.setdefault((k1, k2, kind), []).append((-score, r, k, i, j))
                ends.setdefault(k1, [[], []])[0].append(1)
                ends.setdefault(k2, [[], []])[0].append(1)
            else:
                ends.setdefault(k1, [[], []])[1].append((-score, r, k, i))
    for group in pairs.values():
        for _, r, _, i, j in sorted(group)[1:]:          # the best: highest score, then earliest
            marked |= {(r, i), (r, j)}
    for paired_ends, frags in ends.values():
        for _, r, _, i in sorted(frags)[0 if paired_ends else 1:]:
            marked.add((r, i))
    return marked


def mark(runs, paired: bool, n_ref: int):
    return resolve([entries(recs, paired, n_ref) for recs in runs])


def set_flags(recs, indices):
    out = list(recs)
    for i in indices:
        r = out[i]
        out[i] = r[:18] + struct.pack("<H", struct.unpack_from("<H", r, 18)[0] | 0x400) + r[20:]
    return out


def counts(runs_entries, marked):
    """(pairs, duplicate pairs, fragments, duplicate fragments, marked records)"""
    p = dp = f = df = 0
    for r, ents in enumerate(runs_entries):
        for _, _, _, kind, (i, _) in ents:
            if kind:
                p += 1
                dp += (r, i) in marked
            else:
                f += 1
                df += (r, i) in marked
    return p, dp, f, df, len(marked)


def sorted_places(recs, n_ref: int):
    """where[i]: the place of record i after the stable coordinate sort of the run"""
    order = sorted(range(len(recs)), key=lambda i: bsm.key(n_ref, recs[i]))
    where = [0] * len(recs)
    for place, i in enumerate(order):
        where[i] = place
    return where


def pack_entries(ents, where) -> bytes:
    """the entries as moni_bam_dup_t, idx the records' places in the sorted run"""
    return b"".join(struct.pack("<QQIIII", k1, k2, s, kind, where[i], NONE if j is None else where[j]) for k1, k2, s, kind, (i, j) in ents)
