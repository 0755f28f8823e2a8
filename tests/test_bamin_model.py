"""tests/bamin_model.py held against the strict reader of tests/bam_model.py, which was written independently of it: the SAM decoded from a BAM has
the names, sequences and qualities of the model's FASTQ once the strand is restored; and against hand-written expectations."""
from tests import bam_model
from tests import bamin_model as bm
from tests.test_bam_model import golden

COMPLEMENT = bytes.maketrans(b"ACGTMRWSYKVHDBN", b"TGCAKYWSRMBDHVN")


def fastq_from_sam(sam: bytes) -> bytes:
    out = []
    for line in sam.splitlines():
        if line.startswith(b"@"):
            continue
        f = line.split(b"\t")
        flag, seq, qual = int(f[1]), f[9], f[10]
        if flag & 0x900 or seq == b"*":
            continue
        seq = seq.replace(b"=", b"N")
        qual = b'"' * len(seq) if qual == b"*" else qual
        if flag & 0x10:
            seq, qual = seq.translate(COMPLEMENT)[::-1], qual[::-1]
        out.append(b"@" + f[0] + b"\n" + seq + b"\n+\n" + qual + b"\n")
    return b"".join(out)


def test_against_the_decoder_on_aligned_records():
    for name in ("align_small.sam", "pe_small_orphan.sam"):
        header, lines = golden(name)
        raw = bam_model.encode(header, lines)
        assert any(int(l.split(b"\t")[1]) & 0x10 for l in lines.splitlines())          # reverse-strand records are among them
        t1, t2, counts, reason = bm.fastq_of(bm.ubam(raw, 4096), False)
        assert reason == bm.OK and t2 == b"" and t1 == fastq_from_sam(bam_model.decode(raw))
        assert counts["reads"] == t1.count(b"\n") // 4 and counts["records"] == len(lines.splitlines())


def test_the_writer_reads_back_through_the_decoder():
    raw = bm.header(b"@SQ\tSN:c\tLN:100\n", [(b"c", 100)]) + bm.record(b"a", b"ACGTN", bytes([1, 2, 3, 4, 5]), 16, cigar=(5 << 4,), ref=0, pos=3, tags=b"NMC\x01") + \
        bm.record(b"u", b"GG", None, 4)
    body = bytearray(raw)
    # the writer's bin is the unplaced one; the placed record needs reg2bin's
    at = len(bm.header(b"@SQ\tSN:c\tLN:100\n", [(b"c", 100)]))
    body[at + 14:at + 16] = bam_model.reg2bin(3, 8).to_bytes(2, "little")
    sam = bam_model.decode(bytes(body))
    assert sam == b"@SQ\tSN:c\tLN:100\na\t16\tc\t4\t0\t5M\t*\t0\t0\tACGTN\t\"#$%&\tNM:i:1\nu\t4\t*\t0\t0\t*\t*\t0\t0\tGG\t*\n"
    assert bm.Stream().feed(bytes(body), True)["text1"] == b"@a\nNACGT\n+\n&%$#\"\n@u\nGG\n+\n\"\"\n"


def test_by_hand():
    nib = bytes(range(16))
    packed = bytes(nib[i] << 4 | nib[i + 1] for i in range(0, 16, 2))
    raw = bm.header() + bm.record(b"f", b"", bytes(16), 0, nibbles=(16, packed)) + bm.record(b"r", b"", bytes(range(15)), 0x10, nibbles=(15, packed)) + \
        bm.record(b"s", b"AC", bytes(2), 0x100) + bm.record(b"e", b"", b"", 4)
    r = bm.Stream().feed(raw, True)
    assert r["text1"] == b"@f\nNACMGRSVTWYHKDBN\n+\n" + b"!" * 16 + b"\n@r\nVHMDRWABSYCKGTN\n+\n" + bytes(33 + q for q in reversed(range(15))) + b"\n"
    assert (r["records"], r["reads"], r["skipped_secondary"], r["skipped_empty"], r["carried_bytes"]) == (4, 2, 1, 1, 0)


def test_paired_carry_and_reasons():
    h = bm.header()
    a, b, c = bm.record(b"p", b"AC", bytes(2), 0x4D), bm.record(b"p", b"GT", bytes(2), 0x8D), bm.record(b"q", b"TT", bytes(2), 0x4D)
    s = bm.Stream(True)
    r = s.feed(h + a + b + c, False)
    assert (r["text1"], r["text2"], r["records"], r["carried_bytes"]) == (b"@p\nAC\n+\n!!\n", b"@p\nGT\n+\n!!\n", 2, len(c))
    try:
        s.feed(b"", True)
        assert False
    except bm.Bad as e:
        assert (e.index, e.reason) == (2, bm.TRUNCATED)
    assert s.feed(bm.record(b"q", b"AA", bytes(2), 0x8D), True)["text2"] == b"@q\nAA\n+\n!!\n"
    assert bm.fastq_of(bm.ubam(h + a + c), True)[2:] == ({"first_bad_record": 1}, bm.PAIRING)
    assert bm.fastq_of(bm.ubam(b"BAM\x02" + h[4:]), False)[3] == bm.MAGIC
