"""The BAM reader in plain Python, record by record: what moni_bam_in_feed gives for a stream of BAM bytes - the FASTQ text of
the primary records that have bases, the counts, the carry, and for a damaged stream the lowest bad record and its reason.  No project code.
`Stream` is the state of one context (the carry, the header, the records seen) over inflated bytes; `fastq_of` takes a whole BGZF file.
A small record writer (`record`, `header`, `ubam`) makes unaligned and aligned records the SAM encoder of bam_model would not."""
import struct

from tests import inflate_model as im

# moni_bamin_stats_t::bad_record_reason
OK, MAGIC, HEADER, BLOCK_SIZE, FIELDS, PAIRING, TRUNCATED = range(7)
MAX_BLOCK = 1 << 28
BASES = "NACMGRSVTWYHKDBN"          # `=` comes out as N


class Bad(ValueError):
    def __init__(self, index, reason):
        super().__init__("record %d: reason %d" % (index, reason))
        self.index, self.reason = index, reason


# ---- the writer -------------------------------------------------------------------------------------------------------------------------------
def header(text: bytes = b"@HD\tVN:1.6\tSO:unsorted\n", refs=()) -> bytes:
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, ln in refs:
        out += struct.pack("<i", len(name) + 1) + name + b"\x00" + struct.pack("<i", ln)
    return out


def pack_seq(seq: bytes) -> bytes:
    codes = ["=ACMGRSVTWYHKDBN".index(chr(c)) for c in seq] + ([0] if len(seq) & 1 else [])
    return bytes(codes[i] << 4 | codes[i + 1] for i in range(0, len(codes), 2))


def record(name: bytes, seq: bytes, qual=None, flag: int = 4, cigar=(), tags: bytes = b"", ref: int = -1, pos: int = -1, nibbles=None) -> bytes:
    """One record.  qual: bytes of Phred values, or None for 0xFF throughout.  cigar: packed ops.  nibbles: (l_seq, packed bytes) in place of seq."""
    l_seq, packed = (len(seq), pack_seq(seq)) if nibbles is None else nibbles
    q = b"\xff" * l_seq if qual is None else bytes(qual)
    assert len(q) == l_seq
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(name) + 1, 0, 4680, len(cigar), flag, l_seq, -1, -1, 0)
    body += name + b"\x00" + b"".join(struct.pack("<I", o) for o in cigar) + packed + q + tags
    return struct.pack("<i", len(body)) + body


def ubam(raw: bytes, block_size: int = 65280, level: int = 6, eof: bool = True) -> bytes:
    """the BGZF file of the uncompressed BAM `raw`"""
    return im.bgzip(raw, block_size, level, eof=eof)


# ---- the reader ---------------------------------------------------------------------------------------------------------------------------------
def _compl(n: int) -> int:
    return (n & 1) << 3 | (n & 2) << 1 | (n & 4) >> 1 | (n & 8) >> 3


def fastq_record(s: bytes, a: int) -> bytes:
    """the four lines of the (checked) record at s[a]"""
    l_name, n_ops, flag, l_seq = s[a + 12], struct.unpack_from("<H", s, a + 16)[0], struct.unpack_from("<H", s, a + 18)[0], struct.unpack_from("<i", s, a + 20)[0]
    name = s[a + 36:a + 36 + l_name - 1]
    sq = a + 36 + l_name + 4 * n_ops
    nib = [s[sq + (i >> 1)] >> 4 if not i & 1 else s[sq + (i >> 1)] & 15 for i in range(l_seq)]
    q = s[sq + (l_seq + 1) // 2:sq + (l_seq + 1) // 2 + l_seq]
    absent = q[0] == 0xFF
    if flag & 0x10:
        nib, q = [_compl(n) for n in reversed(nib)], q[::-1]
    qual = b'"' * l_seq if absent else bytes((c + 33) & 0xFF for c in q)
    return b"@" + name + b"\n" + "".join(BASES[n] for n in nib).encode() + b"\n+\n" + qual + b"\n"


def _header_end(s: bytes, base: int):
    """where the records start; None: the header is not whole; raises Bad"""
    n = len(s)
    if s[:4] != b"BAM\x01"[:min(4, n)]:
        raise Bad(base, MAGIC)
    if n < 12:
        return None
    l_text = struct.unpack_from("<i", s, 4)[0]
    if l_text < 0:
        raise Bad(base, HEADER)
    at = 8 + l_text
    if at + 4 > n:
        return None
    n_ref = struct.unpack_from("<i", s, at)[0]
    if n_ref < 0:
        raise Bad(base, HEADER)
    at += 4
    for _ in range(n_ref):
        if at + 4 > n:
            return None
        l_name = struct.unpack_from("<i", s, at)[0]
        if l_name < 1:
            raise Bad(base, HEADER)
        at += 8 + l_name
        if at > n:
            return None
    return at


class Stream:
    def __init__(self, paired: bool = False):
        self.paired, self.carry, self.header_done, self.rec_base = paired, b"", False, 0

    def reset(self):
        self.carry, self.header_done, self.rec_base = b"", False, 0

    def feed(self, data: bytes, last: bool = False) -> dict:
        """One call over inflated bytes.  Raises Bad and leaves the stream as it was; else the call's texts and counts."""
        s, base = self.carry + data, self.rec_base
        n, at, done = len(s), 0, self.header_done
        res = dict(text1=b"", text2=b"", records=0, reads=0, skipped_secondary=0, skipped_empty=0, carried_bytes=len(self.carry), header_done=int(done))
        if not data and not last:
            return res
        recs, list_bad = [], None
        if n and not done:
            at = _header_end(s, base)
            done, at = at is not None, at or 0
        if n and done:
            while at + 4 <= n:
                bs = struct.unpack_from("<I", s, at)[0]
                if not 32 <= bs <= MAX_BLOCK:
                    list_bad = Bad(base + len(recs), BLOCK_SIZE)
                    break
                if at + 4 + bs > n:
                    break
                l_name, n_ops, l_seq = s[at + 12], struct.unpack_from("<H", s, at + 16)[0], struct.unpack_from("<i", s, at + 20)[0]
                if l_name < 1 or l_seq < 0 or 32 + l_name + 4 * n_ops + (l_seq + 1) // 2 + l_seq > bs or s[at + 36 + l_name - 1] != 0:
                    list_bad = Bad(base + len(recs), FIELDS)
                    break
                recs.append(at)
                at += 4 + bs
        # selection, in order
        kept, t1, t2, sec, empty, seen, carry_off = [], [], [], 0, 0, len(recs), at
        for r, a in enumerate(recs):
            flag, l_seq = struct.unpack_from("<H", s, a + 18)[0], struct.unpack_from("<i", s, a + 20)[0]
            if flag & 0x900 or l_seq == 0:
                continue
            if self.paired:
                want = 0x80 if len(kept) & 1 else 0x40
                if not flag & 1 or flag & 0xC0 != want:
                    raise Bad(base + r, PAIRING)
                if len(kept) & 1:
                    b = recs[kept[-1]]
                    if s[b + 12] != s[a + 12] or s[b + 36:b + 36 + s[b + 12]] != s[a + 36:a + 36 + s[a + 12]]:
                        raise Bad(base + r, PAIRING)
            kept.append(r)
        if list_bad:
            raise list_bad
        if self.paired and len(kept) & 1:
            seen = kept.pop()
            carry_off = recs[seen]
        for r in range(seen):
            flag, l_seq = struct.unpack_from("<H", s, recs[r] + 18)[0], struct.unpack_from("<i", s, recs[r] + 20)[0]
            sec += 1 if flag & 0x900 else 0
            empty += 1 if not flag & 0x900 and l_seq == 0 else 0
        if last and carry_off < n:
            raise Bad(base + seen, TRUNCATED)
        for j, r in enumerate(kept):
            (t2 if self.paired and j & 1 else t1).append(fastq_record(s, recs[r]))
        self.carry, self.header_done, self.rec_base = s[carry_off:], done, base + seen
        res.update(text1=b"".join(t1), text2=b"".join(t2), records=seen, reads=len(kept), skipped_secondary=sec, skipped_empty=empty,
                   carried_bytes=n - carry_off, header_done=int(done))
        return res


COUNTS = ("records", "reads", "skipped_secondary", "skipped_empty")


def fastq_of(bam: bytes, paired: bool = False):
    """A whole BGZF file in one call with last set: (text1, text2, counts: COUNTS as a dict, first reason) - on a bad record the texts are
    empty and the counts hold `first_bad_record`."""
    m = im.inflate(bam)
    assert m["bad_blocks"] == 0
    try:
        r = Stream(paired).feed(m["text"], True)
    except Bad as e:
        return b"", b"", {"first_bad_record": e.index}, e.reason
    return r["text1"], r["text2"], {k: r[k] for k in COUNTS}, OK
