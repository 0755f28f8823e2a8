"""tests/bam_model.py against the SAM specification: two records assembled from section 4.2 by hand, reg2bin (5.3) at the level boundaries,
the two halves of the model against each other on the golden SAM files, and the strict reader against damaged copies."""
import os
import struct

import pytest

from tests import bam_model as bam

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SAMS = ("align_small.sam", "align_small_lifted.sam", "pe_small.sam", "pe_small_orphan.sam")
PE_HEADER = b"@SQ\tSN:chr19\tLN:59128983\n"          # the paired golden files carry no header


def golden(name: str):
    """(header, records) of a golden SAM file"""
    h, lines = bam.split_sam(open(os.path.join(GOLDEN, name), "rb").read())
    return h or PE_HEADER, lines


H2 = b"@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:248956422\n@SQ\tSN:chr19\tLN:58617616\n"
H1 = b"@SQ\tSN:chr1\tLN:248956422\n"
KNOWN = [
    (H2, b"r1 16 chr19 16384 60 2S3M1D2M = 17000 -620 ACGTNAC IIIII#I AS:i:-129 NM:i:1 MD:Z:3^A2 AA:Z:".replace(b" ", b"\t") + b"\n",
     "5300000001000000ff3f0000033c49020400100007000000010000006742000094fdffff723100240000003000000012000000200000001248f120282828282802284153737fff"
     "4e4d43014d445a335e41320041415a00"),
    (H1, b"g3 4 * 0 255 * = 0 0 ACG *".replace(b" ", b"\t") + b"\n",
     "28000000ffffffffffffffff03ff48120000040003000000ffffffffffffffff000000006733001240ffffff"),
]


@pytest.mark.parametrize("k", range(len(KNOWN)))
def test_known_answer_records(k):
    header, line, want = KNOWN[k]
    got = bam.encode_records(header, line)
    assert got.hex() == want
    assert struct.unpack_from("<H", got, 14)[0] == (585, 4680)[k]
    assert bam.decode(bam.encode(header, line)) == header + bam.canonical(line)


def test_header():
    assert bam.encode_header(H2).hex() == ("42414d01" + struct.pack("<i", len(H2)).hex() + H2.hex() + "02000000" + "05000000" + b"chr1\0".hex() +
                                           struct.pack("<i", 248956422).hex() + "06000000" + b"chr19\0".hex() + struct.pack("<i", 58617616).hex())
    assert bam.encode_header(b"") == b"BAM\x01" + bytes(8)
    assert bam.decode(bam.encode_header(H2)) == H2


@pytest.mark.parametrize("name", SAMS)
def test_round_trip_golden(name):
    """decode(encode(x)) is x as a BAM can carry it: the golden files hold lower-case bases and `=` beside `*` (tests/bam_model.canonical)"""
    header, lines = golden(name)
    b = bam.encode(header, lines)
    assert bam.decode(b) == header + bam.canonical(lines)
    # canonical touches RNEXT and SEQ alone, and nothing where there is nothing to touch
    for a, c in zip(lines.splitlines(), bam.canonical(lines).splitlines()):
        fa, fc = a.split(b"\t"), c.split(b"\t")
        assert [x for i, x in enumerate(fa) if i not in (6, 9)] == [x for i, x in enumerate(fc) if i not in (6, 9)]
        assert fa[9].upper() == fc[9] and (fa[6] == fc[6] or (fa[2], fa[6], fc[6]) == (b"*", b"=", b"*"))
    if name == "align_small.sam":
        assert len(bam.encode_records(header, lines)) == 19106 and len(lines) == 23508


@pytest.mark.parametrize("beg,end,want", [(-1, 0, 4680), (0, 1, 4681), (16383, 16385, 585), (16384, 16385, 4682), (131071, 131073, 73),
                                          (1048575, 1048577, 9), (8388607, 8388609, 1), (67108863, 67108865, 0), (536870911, 536870912, 37448)])
def test_reg2bin(beg, end, want):
    assert bam.reg2bin(beg, end) == want


def test_integer_tag_types():
    for v, ty, n in ((-2147483648, "i", 4), (-32769, "i", 4), (-32768, "s", 2), (-129, "s", 2), (-128, "c", 1), (-1, "c", 1), (0, "C", 1), (255, "C", 1),
                     (256, "S", 2), (65535, "S", 2), (65536, "I", 4), (4294967295, "I", 4)):
        rec = bam.encode_records(H1, b"r\t0\tchr1\t1\t0\t*\t*\t0\t0\t*\t*\tXX:i:%d\n" % v)
        assert rec[-n - 1:-n] == ty.encode() and len(rec) == 36 + 2 + 3 + n, v
        assert bam.decode(bam.encode_header(H1) + rec).endswith(b"\tXX:i:%d\n" % v)
    for v in (-2147483649, 4294967296):
        with pytest.raises(bam.BadLine) as e:
            bam.encode_records(H1, b"r\t0\tchr1\t1\t0\t*\t*\t0\t0\t*\t*\tXX:i:%d\n" % v)
        assert (e.value.index, e.value.reason) == (0, bam.TAGINT)


def test_decode_rejects_damage():
    header, line, _ = KNOWN[0]
    good = bam.encode(header, line)
    at = len(bam.encode_header(header))
    assert bam.decode(good) == header + line

    def damaged(offset, new):
        return good[:at + offset] + new + good[at + offset + len(new):]

    cases = {
        "trailing byte": good + b"\x00",
        "cut short": good[:-1],
        "block_size one more": damaged(0, struct.pack("<i", 0x53 + 1)) + b"\x00",          # the Z tag's NUL is no longer the record's last byte
        "block_size one less": damaged(0, struct.pack("<i", 0x53 - 1)),
        "bin of the next level": damaged(14, struct.pack("<H", 4682)),
        "l_read_name one less": damaged(12, b"\x02"),                                    # the name's NUL is missing where it should be
        "name NUL overwritten": damaged(38, b"x"),
        "AS:i:-129 as i": None,
        "magic": b"BAM\x02" + good[4:],
    }
    rec = good[at:]
    wide = rec.replace(b"ASs" + struct.pack("<h", -129), b"ASi" + struct.pack("<i", -129))
    cases["AS:i:-129 as i"] = good[:at] + struct.pack("<i", len(wide) - 4) + wide[4:]
    for what, b in cases.items():
        with pytest.raises(bam.BamError):
            bam.decode(b)
            pytest.fail(what)
    # the last Z tag's NUL dropped, block_size following: the record still ends inside a string
    cut = good[:at] + struct.pack("<i", 0x53 - 1) + rec[4:-1]
    with pytest.raises(bam.BamError):
        bam.decode(cut)
