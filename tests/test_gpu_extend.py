"""Extend mode on the GPU: the SAM text of Ctx.extend_batch / extend_run / `moni-hip-align --extend` is byte-identical to the plain-Python
model (tests/extend_model.py).  A parity check: no tolerance."""
import os
import subprocess

import numpy as np
import pytest

from tests import extend_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "moni_align_amd", "host", "moni-hip-align")


def _ragged(reads):
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer(b"".join(reads), dtype=np.uint8).copy(), offs


def _quals(reads, seed=5):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(35, 74, size=len(r), dtype=np.uint8)) for r in reads]


class Rig:
    def __init__(self, case):
        from moni_align_amd import capi
        from oracle import orc
        self.case = case
        self.oidx = orc.OracleIndex(case.path)
        self.idx = capi.Index(fi=case.fi, device=0)
        self.ctx = capi.Ctx(self.idx)

    def model(self, reads, names, quals, **prm):
        return extend_model.extend_batch(self.oidx, self.case.fi, reads, names, quals, **prm)

    def gpu(self, reads, names, quals, **prm):
        seq, offs = _ragged(reads)
        nm, noff = _ragged(names)
        q = None if quals is None else _ragged(quals)[0]
        return self.ctx.extend_batch(seq, offs, nm, noff, q, **prm)

    def check(self, reads, names, quals, **prm):
        want, wst = self.model(reads, names, quals, **prm)
        got, st = self.gpu(reads, names, quals, **prm)
        if got != want:          # the first differing line, for the log
            g, w = got.split(b"\n"), want.split(b"\n")
            k = next((i for i in range(min(len(g), len(w))) if g[i] != w[i]), min(len(g), len(w)))
            raise AssertionError("line %d differs:\n got %r\nwant %r" % (k, g[k] if k < len(g) else None, w[k] if k < len(w) else None))
        assert (st["reads"], st["extended"], st["records"]) == (wst["reads"], wst["extended"], wst["records"])
        return want, wst, st


@pytest.fixture(scope="module")
def rig(small_case):
    r = Rig(small_case)
    yield r
    r.ctx.close()
    r.idx.close()


@pytest.fixture(scope="module")
def sim400(small_case):
    """400 simulated reads of 100 bp with substitutions and indels, half of them reverse-complemented (make_reads draws the strand)"""
    reads = small_case.synth.make_reads(small_case.pg, 400, 100, seed=11, sub_rate=0.02, indel_rate=0.003)
    rd = [r.tobytes() for r in reads]
    return rd, [b"sim.%d" % i for i in range(len(rd))], _quals(rd)


@pytest.fixture(scope="module")
def sim400_want(rig, sim400):
    return rig.model(*sim400)


def _sub(b: bytes, at: int) -> bytes:
    return b[:at] + bytes([b"ACGT"[(b"ACGT".index(b[at]) + 1) & 3]]) + b[at + 1:]


def test_simulated_reads(rig, sim400, sim400_want):
    want, wst = sim400_want
    assert wst["records"] >= 300          # the comparison is not vacuous
    got, st = rig.gpu(*sim400)
    assert got == want
    assert (st["reads"], st["extended"], st["records"]) == (400, wst["extended"], wst["records"])          # stats equal the model's counts
    assert st["dp_tasks"] > 0 and st["dp_cells"] > 0 and st["t_kernel"] > 0


def test_ragged_batch(rig, small_case):
    text = small_case.text
    n = len(text)
    pg = small_case.pg
    len0 = len(pg.seqs[0])
    last_base = n - (2 * pg.w - 1) - 1          # the last base of the last sequence: behind it only separator bytes up to the end of the text
    assert text[last_base] in b"ACGT" and all(c < 6 for c in text[last_base + 1:])
    rng = np.random.default_rng(17)
    reads = []
    for L in (20, 25, 63, 64, 65, 129, 250):          # 20: below min_len; 25: one exact MEM of min_len
        s = text[700:700 + L]
        reads.append(_sub(s, L // 2) if L >= 63 else s)
    reads.append(text[1500:1600])                                   # one exact MEM, both sides empty
    reads.append(_sub(text[1500:1600], 70))                         # MEM at the read's start: right side only
    reads.append(_sub(text[1500:1600], 30))                         # MEM at the read's end: left side only
    reads.append(text[2000:2050] + b"N" + text[2051:2100])          # an N inside
    reads.append(b"N" * 50)                                         # only N
    reads += [bytes(b"ACGT"[x] for x in rng.integers(0, 4, size=60)) for _ in range(20)]          # match nowhere: no record, the read still counts
    reads.append(_sub(text[0:150], 10))                             # mem_pos = 11 <= ext_len: the left target is text [0, 11) reversed
    reads.append(_sub(text[40:190], 10))                            # mem_pos = 51 <= ext_len
    reads.append(_sub(text[last_base - 119:last_base + 1], 109))    # ends at the text's last base: the right target is cut at n and holds separators only
    reads.append(_sub(text[len0 - 120:len0], 109))                  # ends at a sequence's last base: the right target runs over the separators into the next sequence
    # (separator bytes lie between the sequences, so no read of bases is an exact slice across a boundary)
    lc = bytearray(text[2500:2600]); lc[30] += 32; lc[31] += 32
    reads.append(bytes(lc))                                         # lower-case bases: strand 1 keeps them as they are (complement() is upper-case only)
    rc = extend_model.strand1(text[2500:2600])
    reads.append(rc[:2].lower() + rc[2:])
    reads += [extend_model.strand1(r) for r in reads[2:11]]         # the same shapes on strand 1
    names = [b"rag/%d" % i for i in range(len(reads))]
    want, wst, st = rig.check(reads, names, None)
    assert b"rag/0\t" not in want and b"rag/1\t0\t" in want and b"rag/7\t0\t" in want and b"rag/11\t" not in want
    assert wst["reads"] == len(reads) and 20 <= wst["extended"] < len(reads) - 20
    rig.check(reads, names, _quals(reads, seed=8))


def test_indels_beside_the_mem(rig, small_case):
    """a 7-base insertion and a 9-base deletion, 12 bases from the MEM (a substitution bounds it: the 12 M of that side merge into the MEM's) and
    directly at its edge (the side's CIGAR then need not start with M: no merge), on either side and on either strand"""
    text = small_case.text
    ins = b"GATTACA"
    T = lambda a, b: text[1000 + a:1000 + b]
    reads = [
        T(0, 30) + ins + _sub(T(30, 42), 11) + T(42, 112) + _sub(T(112, 124), 0) + T(133, 163),          # 30M 7I 12M | 70 | 12M 9D 30M
        T(0, 30) + _sub(T(39, 51), 11) + T(51, 121) + _sub(T(121, 133), 0) + ins + T(133, 163),          # deletion left, insertion right
        T(0, 30) + ins + T(30, 100) + T(109, 139),          # indels directly at the MEM's edges
        T(0, 30) + T(39, 109) + ins + T(109, 139),
        _sub(T(200, 260), 29) + T(260, 300),                # a substitution directly beside the MEM, on its left
        T(200, 260) + _sub(T(260, 300), 0),                 # ... and on its right
    ]
    reads += [extend_model.strand1(r) for r in reads]
    names = [b"indel.%d" % i for i in range(len(reads))]
    want, wst, _ = rig.check(reads, names, _quals(reads))
    assert wst["records"] >= len(reads) and b"I" in want.split(b"\n")[0].split(b"\t")[5] and b"D" in want.split(b"\n")[0].split(b"\t")[5]


def test_chunking_run_and_empty(rig, sim400, sim400_want):
    want, wst = sim400_want
    reads, names, quals = sim400
    os.environ["MONI_EXTEND_CHUNK"] = "64"
    try:
        got, st = rig.gpu(reads, names, quals)
    finally:
        del os.environ["MONI_EXTEND_CHUNK"]
    assert got == want and st["records"] == wst["records"]
    seq, offs = _ragged(reads)
    nm, noff = _ragged(names)
    rig.ctx.upload(seq, offs)
    got_run, st_run = rig.ctx.extend_run(nm, noff, _ragged(quals)[0])
    assert got_run == want and st_run["extended"] == wst["extended"]
    empty, st0 = rig.ctx.extend_batch(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint8), np.zeros(1, np.uint64), None)
    assert empty == b"" and st0["reads"] == 0 and st0["records"] == 0


def test_non_default_parameters(rig, sim400):
    reads, names, quals = sim400
    prm = dict(min_len=40, ext_len=60, smatch=1, smismatch=3, gapo=6, gape=1)
    want, wst, _ = rig.check(reads[:200], names[:200], quals[:200], **prm)
    assert wst["records"] >= 100


def test_cli_extend(medium_case, tmp_path):
    import __graft_entry__
    from oracle import orc
    __graft_entry__.build()
    N, L = 1500, 150
    reads = medium_case.synth.make_reads(medium_case.pg, N, L, seed=46)
    fq = str(tmp_path / "reads.fastq")
    medium_case.synth.write_fastq(fq, reads)
    out = str(tmp_path / "ext.sam")
    r = subprocess.run([EXE, medium_case.path[:-4], "-p", fq, "-o", out, "--extend", "--gpu-batch", "400", "-t", "4"], capture_output=True)
    assert r.returncode == 0, r.stderr
    o = orc.OracleIndex(medium_case.path)
    names, noff = orc.make_names(N)
    hdr = orc.align_batch(o, reads[:0].reshape(-1), np.zeros(1, np.uint64), names[:0], noff[:1], None, with_header=True)[0]
    want, wst = extend_model.extend_batch(o, medium_case.fi, [x.tobytes() for x in reads], [b"simulated.%d" % i for i in range(N)], [b"I" * L] * N)
    assert wst["records"] >= N // 2
    assert open(out, "rb").read() == hdr + want
    assert b"Number of extended reads: %d/%d" % (wst["extended"], N) in r.stdout
