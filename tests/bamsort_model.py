"""Coordinate-sorted BAM and its .bai index as the SAM specification (4.2, 5.2, 5.3) and this project's DESIGN.md 7.14 fix them, in plain Python
over the standard library, tests/bgzf_model and tests/bam_model's reader.  No project code.  Two halves written independently of each other:

  sort, bai_build   the writer's side, straight from the definitions: the key, a stable sort, the bins, the linear index, the virtual offsets
  bai_query         a strict reader that follows the specification's query (reg2bins, the chunks cut by the linear index, a seek by virtual
                    offset, records until pos >= end) and rejects an index that is not well-formed

A position of -1 on a placed record counts as 0 for the windows of the linear index (and n_intv is at least 1 for a reference with records)."""
import bisect
import struct

from tests import bam_model as bam
from tests import bgzf_model as bgzf

PSEUDO_BIN = 37450


class BaiError(ValueError):
    pass


# ---- records ------------------------------------------------------------------------------------------------------------------------------

def split_records(records: bytes):
    """the records of a raw stream, each with its block_size field"""
    out, at = [], 0
    while at < len(records):
        if len(records) - at < 4:
            raise bam.BamError("%d bytes behind the last record" % (len(records) - at))
        size = struct.unpack_from("<i", records, at)[0]
        if size < 32 or at + 4 + size > len(records):
            raise bam.BamError("block_size %d at %d" % (size, at))
        out.append(records[at:at + 4 + size])
        at += 4 + size
    return out


def fields(rec: bytes):
    """(ref_id, pos, end, bin, flag) of one record: end = pos + the M/D/N/=/X lengths, at least pos + 1"""
    ref, pos, l_name, _, bin_, n_ops, flag = struct.unpack_from("<iiBBHHH", rec, 4)
    reflen = 0
    for k in range(n_ops):
        v = struct.unpack_from("<I", rec, 36 + l_name + 4 * k)[0]
        if bam.OPS[v & 15] in "MDN=X":
            reflen += v >> 4
    return ref, pos, min(pos + max(reflen, 1), 2 ** 31 - 1), bin_, flag


def key(n_ref: int, rec: bytes) -> int:
    ref, pos, _, _, flag = fields(rec)
    return (n_ref if ref < 0 else ref) << 33 | (pos + 1) << 1 | (flag >> 4 & 1)


def sort_list(n_ref: int, recs):
    return sorted(recs, key=lambda r: key(n_ref, r))          # sorted is stable


def sort(header: bytes, records: bytes) -> bytes:
    """the records in samtools sort's order: reference (unplaced last), position, forward before reverse; ties keep input order"""
    return b"".join(sort_list(len(bam.references(header)), split_records(records)))


def coordinate_header(header: bytes) -> bytes:
    return header.replace(b"SO:unknown", b"SO:coordinate", 1)


# ---- a BAM file: blocks, the stream, virtual offsets -------------------------------------------------------------------------------------

class BamFile:
    """the BGZF blocks of a file (walked strictly), its uncompressed stream, its header and where every record begins"""

    def __init__(self, data: bytes, block_size: int = bgzf.MAX_INPUT):
        raws = [r for r, _ in bgzf.walk(data, block_size)]
        self.coff, self.ustart, at, u = [], [], 0, 0
        for r in raws:
            self.coff.append(at)
            self.ustart.append(u)
            at += struct.unpack_from("<H", data, at + 16)[0] + 1
            u += len(r)
        if at != len(data) or not raws or raws[-1] != b"" or not data.endswith(bgzf.EOF_BLOCK):
            raise bam.BamError("the file does not end in the end-of-file block")
        self.raws = raws
        self.stream = b"".join(raws)
        self._full = [b for b, r in enumerate(raws) if r]          # the blocks that hold bytes, for the searches below
        self._full_start = [self.ustart[b] for b in self._full]
        self._at = {c: b for b, c in enumerate(self.coff)}
        s = self.stream
        if s[:4] != b"BAM\x01":
            raise bam.BamError("magic")
        l_text = struct.unpack_from("<i", s, 4)[0]
        self.text = s[8:8 + l_text]
        self.n_ref = struct.unpack_from("<i", s, 8 + l_text)[0]
        at = 12 + l_text
        for _ in range(self.n_ref):
            at += 8 + struct.unpack_from("<i", s, at)[0]
        self.first = at
        self.recs = split_records(s[at:])
        self.starts = []
        for r in self.recs:
            self.starts.append(at)
            at += len(r)

    def voff(self, x: int) -> int:
        """the virtual offset of stream byte x: the block that holds it (for the end of the stream: the end-of-file block)"""
        if not 0 <= x <= len(self.stream):
            raise bam.BamError("no block holds byte %d" % x)
        b = len(self.raws) - 1 if x == len(self.stream) else self._full[bisect.bisect_right(self._full_start, x) - 1]
        return self.coff[b] << 16 | (x - self.ustart[b])

    def seek(self, v: int) -> int:
        """the stream byte of a virtual offset; strict: the block must begin there and hold the byte (or be the end-of-file block)"""
        c, u = v >> 16, v & 0xFFFF
        if c not in self._at:
            raise BaiError("virtual offset %x: no block begins at %d" % (v, c))
        b = self._at[c]
        if u > len(self.raws[b]) or (u == len(self.raws[b]) and b != len(self.raws) - 1):
            raise BaiError("virtual offset %x: the block has %d bytes" % (v, len(self.raws[b])))
        return self.ustart[b] + u


def bai_build(data: bytes, block_size: int = bgzf.MAX_INPUT) -> bytes:
    """the .bai of a coordinate-sorted BAM file, from 5.2 and DESIGN.md 7.14: no merging of adjacent chunks, no folding of bins"""
    f = BamFile(data, block_size)
    refs = [dict(bins={}, lin={}, first=None, last=None, mapped=0, unmapped=0) for _ in range(f.n_ref)]
    no_coor = 0
    cur = None          # (ref, bin, beg, end) of the chunk that is open
    vo = {}

    def v(x):
        if x not in vo:
            vo[x] = f.voff(x)
        return vo[x]

    def close():
        if cur is not None:
            refs[cur[0]]["bins"].setdefault(cur[1], []).append((cur[2], cur[3]))

    for rec, at in zip(f.recs, f.starts):
        ref, pos, end, bin_, flag = fields(rec)
        if ref < 0:
            close()
            cur = None
            no_coor += 1
            continue
        v0, v1 = v(at), v(at + len(rec))
        if cur is not None and cur[0] == ref and cur[1] == bin_:
            cur = (ref, bin_, cur[2], v1)
        else:
            close()
            cur = (ref, bin_, v0, v1)
        R = refs[ref]
        if R["first"] is None:
            R["first"] = v0
        R["last"] = v1
        R["unmapped" if flag & 4 else "mapped"] += 1
        for w in range(max(pos, 0) >> 14, (max(end - 1, 0) >> 14) + 1):
            R["lin"][w] = min(R["lin"].get(w, v0), v0)
    close()
    out = [b"BAI\x01", struct.pack("<i", f.n_ref)]
    for R in refs:
        if R["first"] is None:
            out.append(struct.pack("<ii", 0, 0))
            continue
        out.append(struct.pack("<i", len(R["bins"]) + 1))
        for b in sorted(R["bins"]):
            out.append(struct.pack("<Ii", b, len(R["bins"][b])))
            out += [struct.pack("<QQ", c0, c1) for c0, c1 in R["bins"][b]]
        out.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, R["first"], R["last"], R["mapped"], R["unmapped"]))
        n_intv = max(R["lin"]) + 1
        out.append(struct.pack("<i", n_intv))
        lin, above = [0] * n_intv, 0
        for w in range(n_intv - 1, -1, -1):
            above = R["lin"].get(w, above)
            lin[w] = above
        out += [struct.pack("<Q", x) for x in lin]
    out.append(struct.pack("<Q", no_coor))
    return b"".join(out)


# ---- the reader's side --------------------------------------------------------------------------------------------------------------------

def reg2bins(beg: int, end: int):
    """SAM specification 5.3: the bins that may hold records overlapping [beg, end)"""
    end -= 1
    bins = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        bins += range(first + (beg >> shift), first + (end >> shift) + 1)
    return bins


def bai_parse(bai: bytes):
    """[(bins: {bin: [(beg, end)]}, linear: [ioffset], meta or None)] per reference, and n_no_coor; strict"""
    if bai[:4] != b"BAI\x01":
        raise BaiError("magic")
    at = 4

    def num(fmt):
        nonlocal at
        if at + struct.calcsize("<" + fmt) > len(bai):
            raise BaiError("the index ends inside a field at %d" % at)
        val = struct.unpack_from("<" + fmt, bai, at)[0]
        at += struct.calcsize("<" + fmt)
        return val

    refs = []
    for _ in range(num("i")):
        bins, meta, last_bin = {}, None, -1
        for _ in range(num("i")):
            b, n_chunk = num("I"), num("i")
            chunks = [(num("Q"), num("Q")) for _ in range(n_chunk)]
            if b <= last_bin or b in bins:
                raise BaiError("bin %d behind bin %d" % (b, last_bin))
            last_bin = b
            if b == PSEUDO_BIN:
                if n_chunk != 2:
                    raise BaiError("the pseudo-bin has %d chunks" % n_chunk)
                meta = chunks
                continue
            if b > 37448 or not chunks:
                raise BaiError("bin %d with %d chunks" % (b, n_chunk))
            for k, (c0, c1) in enumerate(chunks):
                if c0 >= c1:
                    raise BaiError("bin %d: a chunk of no span, %x .. %x" % (b, c0, c1))
                if k and c0 < chunks[k - 1][1]:
                    raise BaiError("bin %d: chunks out of order" % b)
            bins[b] = chunks
        linear = [num("Q") for _ in range(num("i"))]
        if bins and meta is None:
            raise BaiError("a reference with bins and no pseudo-bin")
        refs.append((bins, linear, meta))
    no_coor = num("Q")
    if at != len(bai):
        raise BaiError("%d bytes behind the index" % (len(bai) - at))
    return refs, no_coor


def bai_query(bai: bytes, data: bytes, ref: int, beg: int, end: int, block_size: int = bgzf.MAX_INPUT):
    """the records of reference `ref` that overlap [beg, end), in file order, found through the index alone"""
    refs, _ = bai_parse(bai)
    f = BamFile(data, block_size)
    if len(refs) != f.n_ref or not 0 <= ref < f.n_ref:
        raise BaiError("the index has %d references, the file %d" % (len(refs), f.n_ref))
    bins, linear, _ = refs[ref]
    w = beg >> 14
    if w >= len(linear):
        return []          # n_intv reaches the largest end: nothing lies this far right
    min_off = linear[w]
    by_start = {s: k for k, s in enumerate(f.starts)}
    found = {}
    for b in reg2bins(beg, end):
        for c0, c1 in bins.get(b, ()):
            cut = c1 <= min_off          # the linear index says nothing in this chunk reaches the region: checked, not believed
            at, stop = f.seek(c0), f.seek(c1)
            while at < stop:
                if at not in by_start:
                    raise BaiError("bin %d: a chunk begins inside a record, at %d" % (b, at))
                rec = f.recs[by_start[at]]
                r, pos, e, bin_, _ = fields(rec)
                if r != ref or bin_ != b or bam.reg2bin(pos, e) != b:
                    raise BaiError("bin %d of reference %d holds a record of reference %d that reg2bin puts into bin %d" % (b, ref, r, bam.reg2bin(pos, e)))
                for ww in range(max(pos, 0) >> 14, (max(e - 1, 0) >> 14) + 1):
                    if ww >= len(linear) or linear[ww] > f.voff(at):
                        raise BaiError("window %d: the linear index points behind a record that overlaps it" % ww)
                if pos >= end:
                    break
                if e > beg:
                    if cut:
                        raise BaiError("window %d: the linear index cuts a chunk that holds a record of the region" % w)
                    found[at] = rec
                at += len(rec)
            else:
                if at != stop:
                    raise BaiError("bin %d: a chunk ends inside a record" % b)
    return [found[k] for k in sorted(found)]


def brute_query(data: bytes, ref: int, beg: int, end: int, block_size: int = bgzf.MAX_INPUT):
    f = BamFile(data, block_size)
    return [r for r in f.recs if fields(r)[0] == ref and fields(r)[1] < end and fields(r)[2] > beg]
