"""bam_line and the newline passes (moni_align_amd/csrc/bam_core.h: what the BAM encoder's kernels run per line and per tile) replayed on the
host, lanes as loops and passes in launch order, against tests/bam_model.encode byte for byte; every class of bad line gives its reason and
the lowest index.  The real kernels are held to the replay's bytes under -m gpu (tests/test_gpu_bam.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from moni_align_amd import capi
from tests import bam_model as bam
from tests.test_bam_model import H1, H2, KNOWN, SAMS, golden

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sim")
EINVAL = -22
_lib = None

HEADER = b"@HD\tVN:1.6\tSO:unknown\n@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chr10\tLN:2000000000\n@CO\tbetween\n@SQ\tLN:600000000\tSN:chr19\n"


def sim_lib():
    """tests/host_sim/libbam_sim.so, built beside the host-sim library and leaving it alone"""
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "libbam_sim.so")
        src = os.path.join(HERE, "bam_sim.cpp")
        deps = [src, os.path.join(capi.CSRC, "bam_core.h"), os.path.join(os.path.dirname(capi.HERE), "include", "moni_hip.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
        L = C.CDLL(so)
        L.bamsim_header.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.bamsim_records.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
        L.bamsim_reg2bin.argtypes = [C.c_int64, C.c_int64]
        L.bamsim_reg2bin.restype = C.c_uint32
        L.bamsim_base4.argtypes = [C.c_uint32]
        L.bamsim_base4.restype = C.c_uint32
        _lib = L
    return _lib


STAT_KEYS = ("lines", "bam_bytes", "bad_lines", "first_bad_line", "bad_reason")


def sim_header(header: bytes):
    out, n = np.zeros(len(header) * 2 + 64, dtype=np.uint8), C.c_uint64()
    rc = sim_lib().bamsim_header(header, len(header), out.ctypes.data, out.size, C.byref(n))
    return rc, out[:n.value].tobytes() if rc == 0 else b""


def sim_records(header: bytes, text: bytes):
    """(rc, the replay's records, its stats); the output buffer is exactly as large as the size pass says"""
    n, st = C.c_uint64(), np.zeros(5, dtype=np.uint64)
    rc = sim_lib().bamsim_records(header, len(header), text, len(text), None, 0, C.byref(n), st.ctypes.data)
    out = np.zeros(max(n.value, 1), dtype=np.uint8)
    if rc == -34 and n.value:          # MONI_ERANGE: the records did not fit into no room
        rc = sim_lib().bamsim_records(header, len(header), text, len(text), out.ctypes.data, n.value, C.byref(n), st.ctypes.data)
    return rc, out[:n.value].tobytes() if rc == 0 else b"", dict(zip(STAT_KEYS, (int(x) for x in st)))


def sam_line(qname=b"r", flag=0, rname=b"chr19", pos=100, mapq=60, cigar=None, rnext=b"*", pnext=0, tlen=0, seq=b"ACGT", qual=None, tags=()):
    if qual is None:
        qual = b"*" if seq == b"*" else b"I" * len(seq)
    if cigar is None:
        cigar = b"*" if seq == b"*" or rname == b"*" else b"%dM" % len(seq)
    return b"\t".join([qname, b"%d" % flag, rname, b"%d" % pos, b"%d" % mapq, cigar, rnext, b"%d" % pnext, b"%d" % tlen, seq, qual] + list(tags)) + b"\n"


def bases(n: int, seed: int = 0) -> bytes:
    return bytes(np.frombuffer(b"ACGTN", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 5, size=n)])


TAG_INTS = (-2147483648, -32769, -32768, -129, -128, -1, 0, 255, 256, 65535, 65536, 4294967295)
BIN_EDGES = ((-1, 0), (0, 1), (16383, 16385), (16384, 16385), (131071, 131073), (1048575, 1048577), (8388607, 8388609), (67108863, 67108865),
             (536870911, 536870912))


def edge_lines():
    """the issue's edge set, every line valid under HEADER: the smallest shapes at which a 64-byte step, a nibble or a type boundary can go wrong"""
    out = [sam_line(seq=b"*"), sam_line(seq=b"*", rname=b"*", pos=0, flag=4)]
    for n in (1, 2, 63, 64, 65, 127, 129):
        out.append(sam_line(seq=bases(n, n), tags=(b"NM:i:0",)))
        out.append(sam_line(seq=bases(n, n + 1), qual=b"*"))
    out.append(b"q\t4\t*\t0\t0\t*\t*\t0\t0\tA\t#\n")                                                   # shorter than 64 bytes, 11 fields, no tag
    for pad in range(60, 70):                                                                         # SEQ, QUAL and a tag cross a multiple of 64 at every phase
        out.append(sam_line(qname=b"n" * (pad - 40), seq=bases(70, pad), tags=(b"MD:Z:" + b"7" * 70, b"AS:i:-300", b"AA:Z:")))
    out += [sam_line(qname=b"x"), sam_line(qname=b"y" * 254, rname=b"chr1")]
    out += [sam_line(cigar=b"4M"), sam_line(cigar=b"1M1I" * 35, seq=bases(70, 3)), sam_line(cigar=b"268435455M"), sam_line(cigar=b"1S1M1=1X1D1N1I1H1P")]
    out += [sam_line(tags=(b"XI:i:%d" % v,)) for v in TAG_INTS]
    out += [sam_line(tags=tuple(b"X%c:i:%d" % (65 + i, v) for i, v in enumerate(TAG_INTS)))]
    out += [sam_line(tags=(b"ZE:Z:",)), sam_line(tags=(b"ZL:Z:" + bytes(range(48, 123)) * 2 + b"x" * 50, b"XA:A:!", b"ZE:Z:", b"XB:A:~"))]
    out += [sam_line(rname=r, rnext=x, pnext=7) for r in (b"chr1", b"chr10", b"chr19") for x in (b"=", b"*", b"chr10")]
    out += [sam_line(rname=b"*", rnext=b"=", pos=0), sam_line(rname=b"*", rnext=b"*", pos=0), sam_line(rname=b"*", rnext=b"chr1", pos=0, pnext=5)]
    out += [sam_line(rname=b"chr10", pos=beg + 1, cigar=b"%dM" % (end - beg) if end - beg > 0 else b"*") for beg, end in BIN_EDGES if beg >= 0]
    out += [sam_line(rname=b"chr10", pos=0), sam_line(rname=b"chr10", pos=16384, cigar=b"2S"), sam_line(rname=b"chr10", pos=2147483647, tlen=-2147483647, pnext=2147483647)]
    out += [sam_line(seq=b"acgtn.=RYKMSWBDHVUx", flag=65535, mapq=255, tlen=2147483647)]
    return out


def random_lines(n: int, seed: int):
    rng = np.random.default_rng(seed)
    names = (b"chr1", b"chr10", b"chr19")
    out = []
    for i in range(n):
        l = int(rng.choice((0, 1, 2, 30, 63, 64, 65, 100, 150, 151, 250)))
        seq = bases(l, seed + i) if l else b"*"
        mapped = rng.random() < 0.8
        ops = b"".join(b"%d%c" % (int(rng.integers(1, 200)), b"MIDNSHP=X"[int(rng.integers(0, 9))]) for _ in range(int(rng.integers(1, 6))))
        tags = []
        for k in range(int(rng.integers(0, 6))):
            kind = int(rng.integers(0, 3))
            if kind == 0:
                tags.append(b"I%c:i:%d" % (97 + k, int(rng.choice(TAG_INTS)) if rng.random() < 0.3 else int(rng.integers(-70000, 70000))))
            elif kind == 1:
                tags.append(b"Z%c:Z:" % (97 + k) + bases(int(rng.integers(0, 90)), i + k))
            else:
                tags.append(b"A%c:A:%c" % (97 + k, int(rng.integers(33, 127))))
        out.append(sam_line(qname=b"read.%d" % int(rng.integers(0, 10 ** int(rng.integers(1, 12)))), flag=int(rng.integers(0, 65536)),
                            rname=names[int(rng.integers(0, 3))] if mapped else b"*", pos=int(rng.integers(1, 1000000000)) if mapped else 0,
                            mapq=int(rng.integers(0, 256)), cigar=ops if mapped else b"*", rnext=(b"=", b"*", b"chr1")[int(rng.integers(0, 3))],
                            pnext=int(rng.integers(0, 1000000)), tlen=int(rng.integers(-100000, 100000)), seq=seq,
                            qual=b"*" if rng.random() < 0.1 or not l else bytes(rng.integers(33, 127, size=l, dtype=np.uint8)), tags=tuple(tags)))
    return out


def cases():
    """(name, header, records): the inputs of the issue; tests/test_gpu_bam.py sends the same ones through the kernels"""
    c = [("known%d" % k, h, line) for k, (h, line, _) in enumerate(KNOWN)]
    c += [(name,) + golden(name) for name in SAMS]
    c += [("edges", HEADER, b"".join(edge_lines())), ("random2000", HEADER, b"".join(random_lines(2000, 17)))]
    c += [("one_short_line", HEADER, b"q\t4\t*\t0\t0\t*\t*\t0\t0\tA\t#\n"), ("empty", HEADER, b"")]
    return c


CASES = cases()

# (name, the bad line, its reason): every class of bad line
BAD = [
    ("at_line", b"@CO\tcomment\n", bam.AT),
    ("ten_fields", b"r\t0\tchr1\t1\t0\t*\t*\t0\t0\tACGT\n", bam.FIELDS),
    ("empty_line", b"\n", bam.FIELDS),
    ("name_255", sam_line(qname=b"n" * 255), bam.QNAME),
    ("empty_name", sam_line(qname=b""), bam.QNAME),
    ("flag_65536", sam_line(flag=65536), bam.INT),
    ("pos_negative", sam_line(pos=-1), bam.INT),
    ("pos_2_31", sam_line(pos=2147483648), bam.INT),
    ("mapq_256", sam_line(mapq=256), bam.INT),
    ("tlen_2_31", sam_line(tlen=-2147483648), bam.INT),
    ("pos_not_a_number", sam_line().replace(b"\t100\t", b"\t1x0\t"), bam.INT),
    ("pos_empty", sam_line().replace(b"\t100\t", b"\t\t"), bam.INT),
    ("pos_30_digits", sam_line().replace(b"\t100\t", b"\t" + b"9" * 30 + b"\t"), bam.INT),
    ("unknown_rname", sam_line(rname=b"chr2"), bam.RNAME),
    ("rname_prefix_of_a_name", sam_line(rname=b"chr"), bam.RNAME),
    ("unknown_rnext", sam_line(rnext=b"chr100"), bam.RNAME),
    ("op_2_28", sam_line(cigar=b"268435456M"), bam.CIGAR),
    ("op_20_digits", sam_line(cigar=b"1" * 20 + b"M"), bam.CIGAR),
    ("op_letter", sam_line(cigar=b"4Q"), bam.CIGAR),
    ("op_without_length", sam_line(cigar=b"M"), bam.CIGAR),
    ("length_without_op", sam_line(cigar=b"4M3"), bam.CIGAR),
    ("empty_cigar", sam_line(cigar=b""), bam.CIGAR),
    ("ops_65536", sam_line(cigar=b"1M" * 65536), bam.CIGAR),
    ("empty_seq", sam_line(seq=b"", qual=b"*"), bam.SEQ),
    ("qual_one_short", sam_line(qual=b"III"), bam.QUAL),
    ("qual_one_long", sam_line(qual=b"IIIII"), bam.QUAL),
    ("qual_beside_no_seq", sam_line(seq=b"*", qual=b"II"), bam.QUAL),
    ("tag_short", sam_line(tags=(b"NM:i",)), bam.TAG),
    ("tag_colon", sam_line(tags=(b"NM-i:1",)), bam.TAG),
    ("tag_empty", sam_line(tags=(b"",)), bam.TAG),
    ("tag_A_two_bytes", sam_line(tags=(b"XA:A:xy",)), bam.TAG),
    ("tag_int_above", sam_line(tags=(b"XI:i:4294967296",)), bam.TAGINT),
    ("tag_int_below", sam_line(tags=(b"XI:i:-2147483649",)), bam.TAGINT),
    ("tag_int_empty", sam_line(tags=(b"XI:i:",)), bam.TAGINT),
    ("tag_int_float", sam_line(tags=(b"XI:i:1.5",)), bam.TAGINT),
    ("tag_f", sam_line(tags=(b"XF:f:1.5",)), bam.TAGTYPE),
    ("tag_H", sam_line(tags=(b"XH:H:1AE301",)), bam.TAGTYPE),
    ("tag_B", sam_line(tags=(b"XB:B:c,1,2",)), bam.TAGTYPE),
]
GOOD_LINES = [sam_line(qname=b"g%d" % i, seq=bases(40 + i, i)) for i in range(9)]


def bad_text(line: bytes, at: int = 5, second: bytes = None, second_at: int = 7):
    """the bad line as line `at` among good ones; a second bad line behind it"""
    lines = list(GOOD_LINES)
    lines.insert(at, line)
    if second is not None:
        lines.insert(second_at, second)
    return b"".join(lines)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_records_equal_the_model(case):
    _, header, lines = case
    want = bam.encode_records(header, lines)
    rc, got, st = sim_records(header, lines)
    assert rc == 0 and st == dict(lines=lines.count(b"\n"), bam_bytes=len(want), bad_lines=0, first_bad_line=0, bad_reason=0)
    assert got == want, "the replay's records differ from the model's (%d and %d bytes)" % (len(got), len(want))
    assert bam.decode(bam.encode_header(header) + got) == header + bam.canonical(lines)


def test_edge_set_is_the_issues():
    """the edge set holds what the issue lists"""
    recs = [l.rstrip(b"\n").split(b"\t") for l in edge_lines()]
    assert {0, 1, 2, 63, 64, 65, 127, 129} <= {0 if f[9] == b"*" else len(f[9]) for f in recs}
    assert {1, 254} <= {len(f[0]) for f in recs} and min(sum(len(x) + 1 for x in f) for f in recs) < 64
    assert any(len(f) == 11 for f in recs) and any(f[5].count(b"M") + f[5].count(b"I") == 70 for f in recs)
    assert {b"*", b"4M", b"268435455M"} <= {f[5] for f in recs}
    assert {b"XI:i:%d" % v for v in TAG_INTS} <= {t for f in recs for t in f[11:]}
    assert any(t == b"ZE:Z:" for f in recs for t in f[11:]) and any(len(t) == 205 for f in recs for t in f[11:])
    assert {(b"*", b"="), (b"*", b"*"), (b"*", b"chr1"), (b"chr19", b"="), (b"chr1", b"chr10")} <= {(f[2], f[6]) for f in recs}
    bins = {bam.reg2bin(beg, end) for beg, end in BIN_EDGES}
    got = {bam.reg2bin(int(f[3]) - 1, int(f[3]) - 1 + max(1, sum(int(n) for n, op in __import__("re").findall(rb"(\d+)([MDN=X])", f[5])))) for f in recs}
    assert bins <= got


def test_header_equals_the_model():
    for h in (H1, H2, HEADER, b"", b"@HD\tVN:1.6\n", golden("align_small.sam")[0]):
        assert sim_header(h) == (0, bam.encode_header(h))
    for h in (b"@SQ\tSN:chr1\n", b"@SQ\tLN:5\n", b"@SQ\tSN:chr1\tLN:0\n", b"@SQ\tSN:chr1\tLN:2147483648\n", b"@SQ\tSN:" + b"n" * 255 + b"\tLN:5\n", b"@SQ\tSN:\tLN:5\n"):
        assert sim_header(h)[0] == EINVAL, h
        assert sim_records(h, GOOD_LINES[0])[0] == EINVAL


def test_names_do_not_alias():
    """chr1 / chr10 / chr19, the last entry of the dictionary included, and many names in a small table"""
    many = b"".join(b"@SQ\tSN:c%d\tLN:%d\n" % (i, 1000 + i) for i in range(300))
    lines = b"".join(sam_line(rname=b"c%d" % i, rnext=b"c%d" % (299 - i)) for i in range(300))
    rc, got, _ = sim_records(many, lines)
    assert rc == 0 and got == bam.encode_records(many, lines)
    for name, want in ((b"chr1", 0), (b"chr10", 1), (b"chr19", 2)):
        rc, got, _ = sim_records(HEADER, sam_line(rname=name, rnext=name))
        assert rc == 0 and int.from_bytes(got[4:8], "little") == want and int.from_bytes(got[24:28], "little") == want


@pytest.mark.parametrize("case", BAD, ids=[b[0] for b in BAD])
def test_bad_lines(case):
    _, line, reason = case
    with pytest.raises(bam.BadLine) as e:
        bam.encode_records(HEADER, bad_text(line))
    assert (e.value.index, e.value.reason) == (5, reason)
    rc, got, st = sim_records(HEADER, bad_text(line))
    assert rc == EINVAL and got == b"" and (st["bad_lines"], st["first_bad_line"], st["bad_reason"]) == (1, 5, reason)
    # alone, first and last
    assert sim_records(HEADER, line)[2]["bad_reason"] == reason
    for at in (0, 9):
        st = sim_records(HEADER, bad_text(line, at))[2]
        assert (st["bad_lines"], st["first_bad_line"], st["bad_reason"]) == (1, at, reason)


def test_two_bad_lines_the_first_counts():
    """the replay takes the lines last to first, so the later bad line is met first: the index is the minimum, the reason that line's"""
    for (_, a, ra), (_, b, rb) in zip(BAD, BAD[1:] + BAD[:1]):
        st = sim_records(HEADER, bad_text(a, 2, b, 8))[2]
        assert (st["bad_lines"], st["first_bad_line"], st["bad_reason"]) == (2, 2, ra)
        with pytest.raises(bam.BadLine) as e:
            bam.encode_records(HEADER, bad_text(a, 2, b, 8))
        assert (e.value.index, e.value.reason) == (2, ra)


def test_missing_final_newline():
    text = bad_text(GOOD_LINES[0])[:-1]
    rc, got, st = sim_records(HEADER, text)
    assert rc == EINVAL and got == b"" and (st["bad_lines"], st["first_bad_line"], st["bad_reason"]) == (1, 9, bam.NEWLINE)
    with pytest.raises(bam.BadLine) as e:
        bam.encode_records(HEADER, text)
    assert (e.value.index, e.value.reason) == (9, bam.NEWLINE)
    assert sim_records(HEADER, b"x")[2]["first_bad_line"] == 0


def test_cut_between_lines():
    header, lines = golden("pe_small.sam")
    whole = sim_records(header, lines)[1]
    for cut in (1, 7, 160):
        at = len(b"".join(lines.splitlines(keepends=True)[:cut]))
        assert sim_records(header, lines[:at])[1] + sim_records(header, lines[at:])[1] == whole


def test_pieces():
    L = sim_lib()
    for c in range(256):
        want = bam.BASES.find(chr(c).upper()) if c < 128 and chr(c).upper() in bam.BASES else 15
        assert L.bamsim_base4(c) == want, c
    for beg, end in BIN_EDGES + ((2147483646, 2147483647), (0, 1 << 29), (5, 1 << 44)):
        assert L.bamsim_reg2bin(beg, end) == bam.reg2bin(beg, end)
    for beg, end, want in ((-1, 0, 4680), (16383, 16385, 585), (536870911, 536870912, 37448)):
        assert L.bamsim_reg2bin(beg, end) == want
