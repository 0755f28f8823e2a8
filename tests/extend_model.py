"""Plain-Python model of extend mode (the legacy `moni extend`): per read and strand the single longest MEM, one ksw2 extension to each
side, one stitched CIGAR, a bowtie2-style MAPQ, one SAM line.  Written from the mode's specification, case by case; it composes what the
oracle already exports, used as is - OracleIndex.ms_lengths (pointers and matching-statistics lengths), orc.extz (ksw_extz2_sse), the flat
index's text / seq_starts / names - and tests/sam_props.md_nm.  TEST INFRASTRUCTURE ONLY.

Semantics, in the order of the code below:
  strands      strand 0 is the read as given, strand 1 its reverse with A<->T, C<->G complemented (upper case only: every other byte stays);
               each strand yields at most one record, strand 0's first; a read without a record writes nothing
  longest MEM  over the pointers / lengths of ms_lengths: the first position whose length is strictly greater than the best so far and
               for which n_Ns < length, n_Ns counting the matched bytes since the last matched byte that is not 'N'; no MEM or
               len < min_len: no record
  contexts     lcs = read[0, idx) reversed, rcs = read[idx + len, L); nt4: A C G T in either case 0..3 (bytes 0..3 themselves, as in lh3's
               table), everything else 4; min_score = int(20 + 8 ln L)
  targets      left: text[mem_pos - E, mem_pos) reversed if mem_pos > E, else text[0, mem_pos) reversed (a deliberate deviation from the
               reference, which reads E - mem_pos bytes from 0); right: from mem_pos + len, E bytes if that start < n - E, else up to n.
               Not clipped at sequence boundaries.  Empty query: side skipped, score 0.  Query but no target: no record.
  scoring      KSW_EZ_EXTZ_ONLY | KSW_EZ_RIGHT, w = -1, zdrop = -1, end_bonus, mat = simple(smatch, -smismatch);
               score = len * smatch + mqe_left + mqe_right; a record iff score > min_score
  record       ref_pos = mem_pos - (mqe_t_left + 1 if lcs else 0); CIGAR = left reversed, len M (merged into an M beside it), right;
               MD / NM over text[ref_pos, ref_pos + spans); RNAME / POS = the sequence of the concatenation that holds ref_pos, offset + 1;
               MAPQ = nosec[int(best * (10 / (max - min_score)) + 0.5)] with max = L * smatch, best = max - score
"""
import math

import numpy as np

from oracle import orc
from tests import sam_props

UNP_NOSEC = [43, 42, 41, 36, 32, 27, 20, 11, 4, 1, 0]
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_NT4 = np.full(256, 4, dtype=np.uint8)
_NT4[:4] = np.arange(4)
for _i, _c in enumerate(b"ACGT"):
    _NT4[_c] = _i
    _NT4[_c + 32] = _i
KSW_NEG_INF = -0x40000000


def strand1(read: bytes) -> bytes:
    return read[::-1].translate(_COMP)


def simple_mat(a: int, b: int) -> np.ndarray:
    a, b = abs(a), -abs(b)
    m = np.zeros((5, 5), dtype=np.int8)
    m[:4, :4] = b
    for i in range(4):
        m[i, i] = a
    return m.reshape(-1)


def longest_mem(oidx, seq: bytes):
    """(mem_pos, mem_len, mem_idx)"""
    ptr, ln = oidx.ms_lengths(seq)
    best = (0, 0, 0)
    n_ns = 0
    carry = 0
    for i in range(len(seq)):
        li = int(ln[i])
        for k in range(i + carry, i + li):          # the bytes this position's loop matched
            n_ns = n_ns + 1 if seq[k] == ord("N") else 0
        if li > best[1] and n_ns < li:
            best = (int(ptr[i]), li, i)
        carry = max(li - 1, 0)
    return best


def cigar_ops(cig):
    return [(int(c) >> 4, b"MID"[int(c) & 0xf:(int(c) & 0xf) + 1]) for c in cig]


def extend_strand(oidx, text: np.ndarray, seq_starts, seq_names, name: bytes, seq: bytes, qual, strand: int, min_len=25, ext_len=100,
                  smatch=2, smismatch=4, gapo=4, gape=2, end_bonus=400):
    """the SAM line of one strand (bytes), or None"""
    n, L, E = len(text), len(seq), ext_len
    mem_pos, mem_len, idx = longest_mem(oidx, seq)
    if mem_len == 0 or mem_len < min_len:
        return None
    codes = _NT4[np.frombuffer(seq, dtype=np.uint8)]
    lcs, rcs = codes[:idx][::-1], codes[idx + mem_len:]
    min_score = int(20 + 8 * math.log(L))
    mat = simple_mat(smatch, smismatch)
    flag = orc.FLAG_EXTZ_ONLY | orc.FLAG_RIGHT
    sides = []
    for q, t in ((lcs, _NT4[text[mem_pos - E:mem_pos] if mem_pos > E else text[:mem_pos]][::-1]),
                 (rcs, _NT4[text[mem_pos + mem_len:mem_pos + mem_len + (E if mem_pos + mem_len + E < n else n - (mem_pos + mem_len))]])):
        if len(q) == 0:
            sides.append(None)
        elif len(t) == 0:
            return None          # ksw2's untouched result: mqe = KSW_NEG_INF
        else:
            sides.append(orc.extz(q, t, flag, 5, mat, gapo, gape, -1, -1, end_bonus))
    left, right = sides
    score = mem_len * smatch + (left["mqe"] if left else 0) + (right["mqe"] if right else 0)
    if not score > min_score:
        return None
    span_l = left["mqe_t"] + 1 if left else 0
    span_r = right["mqe_t"] + 1 if right else 0
    ref_pos = mem_pos - span_l
    cig = [int(c) for c in left["cigar"][::-1]] if left else []
    if cig and (cig[-1] & 0xf) == 0:
        cig[-1] += mem_len << 4
    else:
        cig.append(mem_len << 4)
    if right and len(right["cigar"]):
        r = [int(c) for c in right["cigar"]]
        if (r[0] & 0xf) == 0:
            cig[-1] += r[0]
        else:
            cig.append(r[0])
        cig.extend(r[1:])
    ops = cigar_ops(cig)
    window = text[ref_pos:ref_pos + span_l + mem_len + span_r].tobytes()
    md, nm = sam_props.md_nm(seq, window, ops)
    sid = int(np.searchsorted(np.asarray(seq_starts[:len(seq_names)], dtype=np.uint64), np.uint64(ref_pos), side="right")) - 1
    max_score = L * smatch
    best = max_score - score
    mapq = 44 if best == max_score else UNP_NOSEC[int(float(best) * (10.0 / float(max_score - min_score)) + 0.5)]
    q = b"*" if qual is None else (qual[::-1] if strand else qual)
    return b"\t".join([name, b"16" if strand else b"0", seq_names[sid].encode(), b"%d" % (ref_pos - int(seq_starts[sid]) + 1), b"%d" % mapq,
                       b"".join(b"%d%s" % o for o in ops), b"*", b"0", b"0", seq, q, b"AS:i:%d" % score, b"NM:i:%d" % nm, b"MD:Z:" + md]) + b"\n"


def extend_batch(oidx, fi, reads, names, quals=None, **prm):
    """reads / names / quals: lists of bytes (quals None: no qualities).  Returns (SAM bytes, {"reads", "extended", "records"})."""
    text = np.asarray(fi.text, dtype=np.uint8)
    out = []
    extended = records = 0
    for i, rd in enumerate(reads):
        got = False
        for strand in (0, 1):
            seq = strand1(rd) if strand else rd
            ln = extend_strand(oidx, text, fi.seq_starts, fi.names, names[i], seq, None if quals is None else quals[i], strand, **prm)
            if ln is not None:
                out.append(ln); records += 1; got = True
        extended += got
    return b"".join(out), {"reads": len(reads), "extended": extended, "records": records}
