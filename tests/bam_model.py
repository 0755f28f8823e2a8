"""BAM as the SAM specification (4.2, and 5.3 for the bins) and this project's DESIGN.md 7.12 fix it, in plain Python over the standard library,
as two halves written independently of each other: `encode` (SAM text -> BAM bytes) and `decode` (a strict reader, BAM bytes -> SAM text).
No project code.  What a BAM cannot carry is named by `canonical`: the case of a base, an RNEXT of `=` beside an RNAME of `*` (both are
refID -1 = next_refID, which reads back as `*`), and an RNEXT that spells RNAME out (it reads back as `=`)."""
import struct

# moni_bam_stats_t::bad_reason
OK, NEWLINE, AT, FIELDS, QNAME, INT, RNAME, CIGAR, SEQ, QUAL, TAG, TAGINT, TAGTYPE, LENGTH = range(14)

BASES = "=ACMGRSVTWYHKDBN"
OPS = "MIDNSHP=X"


class BadLine(ValueError):
    def __init__(self, index, reason):
        super().__init__("line %d: reason %d" % (index, reason))
        self.index, self.reason = index, reason


class BamError(ValueError):
    pass


def reg2bin(beg: int, end: int) -> int:
    """SAM specification 5.3 on Python's integers (>> is arithmetic): the bin of [beg, end)"""
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


# ---- encode ----------------------------------------------------------------------------------------------------------------------------

def references(header: bytes):
    """[(name, length)] of the @SQ lines, in order"""
    refs = []
    for line in header.split(b"\n"):
        if line.startswith(b"@SQ\t"):
            sn = [f[3:] for f in line.split(b"\t")[1:] if f.startswith(b"SN:")]
            ln = [f[3:] for f in line.split(b"\t")[1:] if f.startswith(b"LN:")]
            if not sn or not ln or not sn[0] or len(sn[0]) > 254 or not ln[0].isdigit() or not 1 <= int(ln[0]) < 2 ** 31:
                raise BamError("bad @SQ line %r" % line)
            refs.append((sn[0], int(ln[0])))
    return refs


def encode_header(header: bytes) -> bytes:
    refs = references(header)
    out = b"BAM\x01" + struct.pack("<i", len(header)) + header + struct.pack("<i", len(refs))
    for name, ln in refs:
        out += struct.pack("<i", len(name) + 1) + name + b"\x00" + struct.pack("<i", ln)
    return out


def _integer(field: bytes, lo: int, hi: int):
    """-?[0-9]+ within [lo, hi], or None"""
    digits = field[1:] if field.startswith(b"-") else field
    if not digits or any(not 48 <= c <= 57 for c in digits):
        return None
    v = int(field)
    return v if lo <= v <= hi else None


def encode_record(line: bytes, ids: dict, index: int = 0) -> bytes:
    """one line (without its newline) -> one record; raises BadLine(index, reason)"""
    def bad(reason):
        raise BadLine(index, reason)

    if len(line) >= 1 << 28:
        bad(LENGTH)
    if line.startswith(b"@"):
        bad(AT)
    f = line.split(b"\t")
    if len(f) < 11:
        bad(FIELDS)
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
    if not 1 <= len(qname) <= 254:
        bad(QNAME)
    nums = (_integer(flag, 0, 65535), _integer(pos, 0, 2 ** 31 - 1), _integer(mapq, 0, 255), _integer(pnext, 0, 2 ** 31 - 1),
            _integer(tlen, -(2 ** 31 - 1), 2 ** 31 - 1))
    if None in nums:
        bad(INT)
    flag, pos, mapq, pnext, tlen = nums
    if rname == b"*":
        ref = -1
    elif rname in ids:
        ref = ids[rname]
    else:
        bad(RNAME)
    if rnext == b"=":
        nref = ref
    elif rnext == b"*":
        nref = -1
    elif rnext in ids:
        nref = ids[rnext]
    else:
        bad(RNAME)
    ops, reflen = [], 0
    if cigar != b"*":
        if not cigar:
            bad(CIGAR)
        num = b""
        for c in cigar:
            if 48 <= c <= 57:
                num += bytes([c])
                continue
            op = OPS.find(chr(c)) if c < 128 else -1
            if op < 0 or not num or int(num) >= 1 << 28 or len(ops) == 65535:
                bad(CIGAR)
            ops.append(int(num) << 4 | op)
            if chr(c) in "MDN=X":
                reflen += int(num)
            num = b""
        if num:
            bad(CIGAR)
    if not seq:
        bad(SEQ)
    l_seq = 0 if seq == b"*" else len(seq)
    if qual == b"*":
        q = b"\xff" * l_seq
    elif len(qual) != l_seq:
        bad(QUAL)
    else:
        q = bytes((c - 33) & 0xFF for c in qual)
    codes = [BASES.find(chr(c).upper()) if c < 128 and chr(c).upper() in BASES else 15 for c in (seq if l_seq else b"")]
    if l_seq & 1:
        codes.append(0)
    packed = bytes(codes[i] << 4 | codes[i + 1] for i in range(0, len(codes), 2))
    tags = b""
    for t in f[11:]:
        if len(t) < 5 or t[2:3] != b":" or t[4:5] != b":":
            bad(TAG)
        ty, val = t[3:4], t[5:]
        if ty == b"A":
            if len(val) != 1:
                bad(TAG)
            tags += t[:2] + b"A" + val
        elif ty == b"i":
            v = _integer(val, -(2 ** 31), 2 ** 32 - 1)
            if v is None:
                bad(TAGINT)
            if v >= 0:
                tags += t[:2] + (b"C" + struct.pack("<B", v) if v <= 255 else b"S" + struct.pack("<H", v) if v <= 65535 else b"I" + struct.pack("<I", v))
            else:
                tags += t[:2] + (b"c" + struct.pack("<b", v) if v >= -128 else b"s" + struct.pack("<h", v) if v >= -32768 else b"i" + struct.pack("<i", v))
        elif ty == b"Z":
            tags += t[:2] + b"Z" + val + b"\x00"
        else:
            bad(TAGTYPE)
    body = struct.pack("<iiBBHHHiiii", ref, pos - 1, len(qname) + 1, mapq, reg2bin(pos - 1, pos - 1 + max(reflen, 1)) & 0xFFFF, len(ops), flag, l_seq,
                       nref, pnext - 1, tlen)
    body += qname + b"\x00" + b"".join(struct.pack("<I", o) for o in ops) + packed + q + tags
    return struct.pack("<i", len(body)) + body


def encode_records(header: bytes, lines: bytes) -> bytes:
    """the records of `lines` (records only, each ending in a newline); raises BadLine with the lowest bad index"""
    ids = {}
    for i, (name, _) in enumerate(references(header)):
        ids.setdefault(name, i)
    if not lines:
        return b""
    if not lines.endswith(b"\n"):
        raise BadLine(lines.count(b"\n"), NEWLINE)
    return b"".join(encode_record(l, ids, i) for i, l in enumerate(lines[:-1].split(b"\n")))


def split_sam(text: bytes):
    """(the @ lines, the records) of a SAM file"""
    lines = text.splitlines(keepends=True)
    return b"".join(l for l in lines if l.startswith(b"@")), b"".join(l for l in lines if not l.startswith(b"@"))


def encode(header: bytes, lines: bytes) -> bytes:
    """a whole uncompressed BAM: the header, then the records"""
    return encode_header(header) + encode_records(header, lines)


# ---- decode: written from 4.2's table alone, top to bottom -----------------------------------------------------------------------------------

class _Reader:
    def __init__(self, data, at=0, end=None):
        self.d, self.at, self.end = data, at, len(data) if end is None else end

    def take(self, n):
        if n < 0 or self.at + n > self.end:
            raise BamError("%d bytes wanted at %d, %d left" % (n, self.at, self.end - self.at))
        self.at += n
        return self.d[self.at - n:self.at]

    def num(self, fmt):
        return struct.unpack("<" + fmt, self.take(struct.calcsize("<" + fmt)))[0]

    def cstring(self, n=None):
        """n bytes the last of which is the only NUL; or, without n, up to the next NUL"""
        if n is None:
            z = self.d.find(b"\x00", self.at, self.end)
            if z < 0:
                raise BamError("no NUL behind %d" % self.at)
            n = z - self.at + 1
        s = self.take(n)
        if not s or s[-1] != 0 or b"\x00" in s[:-1]:
            raise BamError("a string of %d bytes at %d without its one NUL at the end" % (n, self.at - n))
        return s[:-1]


_INT_TYPES = {"c": ("b", -128, -1), "C": ("B", 0, 255), "s": ("h", -32768, -129), "S": ("H", 256, 65535), "i": ("i", -2 ** 31, -32769), "I": ("I", 65536, 2 ** 32 - 1)}


def decode(bam: bytes) -> bytes:
    """The SAM text of an uncompressed BAM, header first.  Strict: raises BamError on trailing or missing bytes, a block_size that disagrees
    with the record's fields, a bin that is not reg2bin's, an integer tag in a wider type than its value needs, a missing NUL, an id outside
    the dictionary, and on the tag types this project does not write."""
    r = _Reader(bam)
    if r.take(4) != b"BAM\x01":
        raise BamError("magic")
    text = r.take(r.num("i"))
    names = []
    for _ in range(r.num("i")):
        n = r.num("i")
        names.append(r.cstring(n))
        if r.num("i") < 1:
            raise BamError("l_ref")
    if names != [n for n, _ in references(text)]:
        raise BamError("the references are not the header text's @SQ lines")
    out = [text]

    def ref_name(i):
        if not -1 <= i < len(names):
            raise BamError("refID %d" % i)
        return b"*" if i < 0 else names[i]

    while r.at < len(bam):
        size = r.num("i")
        if size < 32 or r.at + size > len(bam):
            raise BamError("block_size %d at %d" % (size, r.at - 4))
        b = _Reader(bam, r.at, r.at + size)
        ref, pos, l_name, mapq, bin_, n_ops, flag, l_seq, nref, npos, tlen = (b.num(c) for c in "iiBBHHHiiii")
        if l_name < 2 or l_seq < 0 or pos < -1 or npos < -1:
            raise BamError("a fixed field out of range at %d" % r.at)
        qname = b.cstring(l_name)
        cigar, reflen = b"", 0
        for _ in range(n_ops):
            v = b.num("I")
            if v & 15 > 8:
                raise BamError("CIGAR op %d" % (v & 15))
            cigar += b"%d%c" % (v >> 4, OPS[v & 15].encode())
            if OPS[v & 15] in "MDN=X":
                reflen += v >> 4
        if bin_ != reg2bin(pos, pos + max(reflen, 1)) & 0xFFFF:
            raise BamError("bin %d at %d: reg2bin gives %d" % (bin_, r.at, reg2bin(pos, pos + max(reflen, 1))))
        packed = b.take((l_seq + 1) // 2)
        if l_seq & 1 and packed[-1] & 15:
            raise BamError("the spare nibble of SEQ is not 0")
        seq = "".join(BASES[packed[i >> 1] >> 4 if not i & 1 else packed[i >> 1] & 15] for i in range(l_seq)).encode()
        q = b.take(l_seq)
        if l_seq and q == b"\xff" * l_seq:
            qual = b"*"
        else:
            if any(c > 93 for c in q):
                raise BamError("a quality above 93")
            qual = bytes(c + 33 for c in q)
        tags = []
        while b.at < b.end:
            name, ty = b.take(2), chr(b.num("B"))
            if ty == "A":
                tags.append(name + b":A:" + b.take(1))
            elif ty == "Z":
                tags.append(name + b":Z:" + b.cstring())
            elif ty in _INT_TYPES:
                fmt, lo, hi = _INT_TYPES[ty]
                v = b.num(fmt)
                if not lo <= v <= hi:
                    raise BamError("tag %s: %d in type %s, a wider one than it needs" % (name.decode(), v, ty))
                tags.append(name + b":i:%d" % v)
            else:
                raise BamError("tag type %r" % ty)
        rnext = b"=" if nref == ref and ref >= 0 else ref_name(nref)
        fields = [qname, b"%d" % flag, ref_name(ref), b"%d" % (pos + 1), b"%d" % mapq, cigar or b"*", rnext, b"%d" % (npos + 1), b"%d" % tlen,
                  seq or b"*", qual if l_seq else b"*"] + tags
        out.append(b"\t".join(fields) + b"\n")
        r.at += size
    return b"".join(out)


def canonical(sam: bytes) -> bytes:
    """`sam` as a BAM can carry it: SEQ in upper case with every byte outside `=ACMGRSVTWYHKDBN` as N, RNEXT `*` where it is `=` beside an RNAME
    of `*`, and `=` where it spells RNAME out.  Everything else - the @ lines, the other fields, the tags and their order - is kept byte for byte."""
    out = []
    for line in sam.splitlines(keepends=True):
        if not line.startswith(b"@"):
            f = line.split(b"\t")
            if f[2] == b"*" and f[6] == b"=":
                f[6] = b"*"
            elif f[6] == f[2] and f[2] != b"*":
                f[6] = b"="
            if f[9] != b"*":
                f[9] = "".join(c if c in BASES else "N" for c in f[9].decode("latin-1").upper()).encode()
            line = b"\t".join(f)
        out.append(line)
    return b"".join(out)
