"""tests/bamsort_model.py against answers assembled by hand, its query against a brute-force scan at the edges of windows and bins, and damaged
indexes, which the strict reader must reject.  The kernels and the library's index builder are held to this model elsewhere
(tests/test_host_bamsort.py, tests/test_gpu_bamsort.py, tests/test_cli_sort.py)."""
import struct

import pytest

from tests import bamsort_model as bsm
from tests import bgzf_model as bgzf
from tests.bamsort_cases import H1, H2, bam_file, block_sizes, record
from tests.bam_model import encode_header

H3 = H2 + b"@SQ\tSN:chr3\tLN:1000\n"


def test_known_sort():
    a = record(ref=1, pos=5, size=50, seed=1)
    b = record(ref=-1, pos=-1, size=41, seed=2)
    c = record(ref=0, pos=16380, flag=16, size=60, seed=3)
    d = record(ref=0, pos=16380, flag=0, size=61, seed=4)
    e = record(ref=0, pos=16380, flag=16, size=62, seed=5)
    f = record(ref=0, pos=-1, size=63, seed=6)
    assert bsm.sort(H2, a + b + c + d + e + f) == f + d + c + e + a + b
    assert bsm.key(2, b) == 2 << 33 and bsm.key(2, c) == 16381 << 1 | 1 and bsm.key(2, a) == 1 << 33 | 6 << 1
    assert bsm.coordinate_header(H2).startswith(b"@HD\tVN:1.6\tSO:coordinate\n@SQ")


def test_known_index():
    """three records over two references, one straddling 16 384, and one unplaced record; every offset worked out by hand"""
    r0 = record(ref=0, pos=100, ops=[(50, "M")], size=100, seed=0)
    r1 = record(ref=0, pos=16380, ops=[(10, "M")], size=90, seed=1)
    r2 = record(ref=1, pos=5, ops=[(1, "M")], size=80, seed=2)
    r3 = record(ref=-1, pos=-1, size=70, seed=3)
    data, chunks = bam_file(H2, [r0, r1, r2, r3], 65280)
    hdr = block_sizes(data)[0]          # the header's one block; the records' block begins behind it
    assert chunks[0][3] == hdr and len(block_sizes(data)) == 3
    v = [hdr << 16 | x for x in (0, 100, 190, 270)]
    end = (len(data) - 28) << 16          # the end-of-file block
    want = b"BAI\x01" + struct.pack("<i", 2)
    want += struct.pack("<i", 3) + struct.pack("<IiQQ", 585, 1, v[1], v[2]) + struct.pack("<IiQQ", 4681, 1, v[0], v[1])
    want += struct.pack("<IiQQQQ", 37450, 2, v[0], v[2], 2, 0) + struct.pack("<iQQ", 2, v[0], v[1])
    want += struct.pack("<i", 2) + struct.pack("<IiQQ", 4681, 1, v[2], v[3]) + struct.pack("<IiQQQQ", 37450, 2, v[2], v[3], 1, 0) + struct.pack("<iQ", 1, v[2])
    want += struct.pack("<Q", 1)
    assert bsm.bai_build(data) == want
    assert bsm.bai_query(want, data, 0, 16384, 16385) == [r1] and bsm.bai_query(want, data, 0, 0, 16384) == [r0, r1] and bsm.bai_query(want, data, 1, 0, 5) == []
    # the last placed record ends where the unplaced one begins; without it, at the end-of-file block
    data2, _ = bam_file(H2, [r0, r1, r2], 65280)
    assert struct.pack("<QQ", v[2], (len(data2) - 28) << 16) in bsm.bai_build(data2) and end != (len(data2) - 28) << 16


def _edge_file():
    recs = []
    for k, edge in enumerate((1 << 14, 1 << 17, 1 << 20, 1 << 23, 1 << 26)):          # a record that straddles each bin level, one on each side of it
        recs += [record(pos=edge - 10, ops=[(10, "M")], size=80 + k, seed=3 * k), record(pos=edge - 5, ops=[(10, "M")], size=90 + k, seed=3 * k + 1),
                 record(pos=edge, ops=[(10, "M")], size=100 + k, seed=3 * k + 2)]
    recs += [record(pos=16383, ops=[(1, "M")], size=70, seed=40), record(pos=16384, ops=[(1, "M")], size=71, seed=41)]
    recs += [record(pos=5 * 16384 + 7, ops=[(3, "M")], size=72, seed=42)]          # windows 2..4 stay empty between 1 and 5
    recs += [record(ref=2, pos=3, ops=[(3, "M")], size=73, seed=43), record(ref=-1, pos=-1, size=74, seed=44)]          # reference 1 has no record
    recs = bsm.sort_list(3, recs)
    return recs, bam_file(H3, recs, 300, chunk_ends=(4, 9))[0]


def test_query_against_brute_force():
    recs, data = _edge_file()
    bai = bsm.bai_build(data, 300)
    refs, no_coor = bsm.bai_parse(bai)
    assert no_coor == 1 and refs[1] == ({}, [], None) and len(refs[0][1]) == 1 + ((1 << 26) + 9 >> 14)
    assert refs[0][1][2] == refs[0][1][3] == refs[0][1][4] == refs[0][1][5]          # empty windows take the next populated one's offset
    regions = [(0, 16383, 16384), (0, 16384, 16385), (0, 16383, 16385), (0, 0, 16383), (0, 2 * 16384, 5 * 16384), (0, 2 * 16384, 5 * 16384 + 8),
               (0, (1 << 26) + 10, (1 << 26) + 500), (0, (1 << 26) + 9, (1 << 26) + 10), (0, 1 << 27, (1 << 27) + 5), (1, 0, 1000), (2, 0, 4), (2, 5, 6), (2, 6, 7),
               (0, 0, 1 << 29)]
    regions += [(0, e - d, e + d) for e in (1 << 14, 1 << 17, 1 << 20, 1 << 23, 1 << 26) for d in (1, 6, 11)]
    for ref, beg, end in regions:
        assert bsm.bai_query(bai, data, ref, beg, end, 300) == bsm.brute_query(data, ref, beg, end, 300), (ref, beg, end)
    assert len(bsm.bai_query(bai, data, 0, 0, 1 << 29, 300)) == len(recs) - 2


def test_damaged_indexes_are_rejected():
    recs, data = _edge_file()
    bai = bsm.bai_build(data, 300)
    q = lambda b: bsm.bai_query(b, data, 0, 0, 1 << 29, 300)
    assert q(bai)
    with pytest.raises(bsm.BaiError):
        q(b"BAI\x02" + bai[4:])
    with pytest.raises(bsm.BaiError):
        q(bai + b"\x00")
    with pytest.raises(bsm.BaiError):
        q(bai[:-1])
    # reference 0's first bin: its chunk made empty, then its two ends swapped
    at = 4 + 4 + 4          # magic, n_ref, n_bin
    b, n_chunk, c0, c1 = struct.unpack_from("<IiQQ", bai, at)
    assert n_chunk >= 1
    for bad in ((c0, c0), (c1, c0)):
        with pytest.raises(bsm.BaiError):
            q(bai[:at + 8] + struct.pack("<QQ", *bad) + bai[at + 24:])
    # a bin with two chunks, the second before the first
    refs, _ = bsm.bai_parse(bai)
    two = [(bb, ch) for bb, ch in refs[0][0].items() if len(ch) >= 2]
    assert two, "the edge file has a bin with two chunks"
    bb, ch = two[0]
    pat = struct.pack("<Ii", bb, len(ch)) + b"".join(struct.pack("<QQ", *c) for c in ch)
    swapped = struct.pack("<Ii", bb, len(ch)) + b"".join(struct.pack("<QQ", *c) for c in [ch[1], ch[0]] + ch[2:])
    assert bai.count(pat) == 1
    with pytest.raises(bsm.BaiError):
        q(bai.replace(pat, swapped))
    # a bin number reg2bin could not give for the records in it: the last bin renumbered to its free neighbour (the bins stay in order)
    big = max(refs[0][0])
    pat = struct.pack("<Ii", big, len(refs[0][0][big]))
    assert big + 1 <= 37448 and bai.count(pat) == 1
    with pytest.raises(bsm.BaiError, match="reg2bin"):
        q(bai.replace(pat, struct.pack("<Ii", big + 1, len(refs[0][0][big]))))
    # a linear-index entry that points behind a record it must reach: window 0 takes the last window's offset
    n_bin = struct.unpack_from("<i", bai, 8)[0]
    p = 12
    for _ in range(n_bin):
        p += 8 + 16 * struct.unpack_from("<i", bai, p + 4)[0]
    n_intv = struct.unpack_from("<i", bai, p)[0]
    last = struct.unpack_from("<Q", bai, p + 4 + 8 * (n_intv - 1))[0]
    with pytest.raises(bsm.BaiError):
        q(bai[:p + 4] + struct.pack("<Q", last) + bai[p + 12:])


def test_file_must_end_in_the_eof_block():
    _, data = _edge_file()
    with pytest.raises(Exception):
        bsm.bai_build(data[:-28], 300)
    assert bgzf.walk(data, 300)[-1][0] == b"" and encode_header(H3) == bsm.BamFile(data, 300).stream[:bsm.BamFile(data, 300).first]
