"""Extend mode without a GPU: properties of the plain-Python model (tests/extend_model.py) that need no code of the kernels - the CIGAR
consumes the read, AS is the score of the path the CIGAR spells over the window RNAME / POS name, MD / NM recompute, the first of two
equally long MEMs wins - and the surface the feature adds: the three exported symbols and the --extend option of moni-hip-align."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import extend_model, sam_props

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "moni_align_amd", "host", "moni-hip-align")


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__
    __graft_entry__.build()
    return EXE


@pytest.fixture(scope="module")
def oidx(small_case):
    from oracle import orc
    return orc.OracleIndex(small_case.path)


def _records(sam: bytes):
    return [ln.split(b"\t") for ln in sam.split(b"\n") if ln]


def test_model_records_are_consistent(small_case, oidx):
    fi, text = small_case.fi, small_case.text
    reads = small_case.synth.make_reads(small_case.pg, 80, 100, seed=7, sub_rate=0.02, indel_rate=0.003)
    names = [b"r%d" % i for i in range(len(reads))]
    quals = [bytes(33 + (7 * i + k) % 40 for k in range(100)) for i in range(len(reads))]
    sam, st = extend_model.extend_batch(oidx, fi, [r.tobytes() for r in reads], names, quals)
    recs = _records(sam)
    assert st["records"] == len(recs) >= 60 and st["extended"] <= st["reads"] == 80
    starts = {n: int(s) for n, s in zip(fi.names, fi.seq_starts)}
    order = []
    for f in recs:
        i = int(f[0][1:])
        order.append((i, int(f[1]) // 16))
        rd = reads[i].tobytes()
        seq = f[9]
        assert int(f[1]) in (0, 16) and seq == (extend_model.strand1(rd) if int(f[1]) else rd)
        assert f[10] == (quals[i][::-1] if int(f[1]) else quals[i]) and f[6:9] == [b"*", b"0", b"0"]
        ops = sam_props.parse_cigar(f[5])
        assert sum(n for n, op in ops if op in (b"M", b"I")) == len(seq) and all(n > 0 for n, _ in ops)          # the CIGAR consumes the whole read
        assert all(a[1] != b[1] for a, b in zip(ops, ops[1:]))                                                     # ... and no operation repeats: M merged
        span = sum(n for n, op in ops if op in (b"M", b"D"))
        at = starts[f[2].decode()] + int(f[3]) - 1                                                                # RNAME, POS locate the window
        window = text[at:at + span]
        tags = {t[:2]: t[5:] for t in f[11:]}
        assert [t[:5] for t in f[11:]] == [b"AS:i:", b"NM:i:", b"MD:Z:"]
        AS = int(tags[b"AS"])
        assert sam_props.path_score(seq, window, ops) == AS
        md, nm = sam_props.md_nm(seq, window, ops)
        assert md == tags[b"MD"] and nm == int(tags[b"NM"])
        L = len(seq)
        min_score = int(20 + 8 * np.log(L))
        assert min_score < AS <= 2 * L
        assert int(f[4]) == extend_model.UNP_NOSEC[int((2 * L - AS) * (10.0 / (2 * L - min_score)) + 0.5)]
    assert order == sorted(order)          # read order, strand 0 before strand 1


def test_first_of_two_equal_mems_wins(small_case, oidx):
    """read = A + B, two text slices of 40 bases from different places that do not extend into each other: both MEMs have length 40 and the
    earlier one (idx 0) is kept - the comparison is strict."""
    text = small_case.text
    rng = np.random.default_rng(3)
    found = None
    for _ in range(200):
        p, q = (int(x) for x in rng.integers(100, 3800, size=2))
        if abs(p - q) < 200:
            continue
        rd = text[p:p + 40] + text[q:q + 40]
        _, ln = oidx.ms_lengths(rd)
        if int(ln[0]) == 40 and int(ln[40]) == 40 and int(ln.max()) == 40:
            found = (rd, p, q)
            break
    assert found is not None
    rd, p, q = found
    pos, ln, idx = extend_model.longest_mem(oidx, rd)
    assert (ln, idx) == (40, 0) and text[pos:pos + 40] == rd[:40]
    line = extend_model.extend_strand(oidx, np.frombuffer(text, np.uint8), small_case.fi.seq_starts, small_case.fi.names, b"t", rd, None, 0)
    if line is not None:          # the record, if the extension passes the threshold, is anchored at A
        f = line.split(b"\t")
        assert sam_props.parse_cigar(f[5])[0][1] == b"M" and f[10] == b"*"


def test_library_exports_extend():
    from moni_align_amd import capi
    capi.build_lib()
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in ("moni_extend_batch", "moni_extend_run", "moni_extend_params_default"):
        assert hasattr(L, name), name
    prm = capi.ExtendParamsC()
    capi.lib().moni_extend_params_default(ctypes.byref(prm))
    assert (prm.min_len, prm.ext_len, prm.smatch, prm.smismatch, prm.gapo, prm.gape, prm.end_bonus, prm.w, prm.zdrop) == (25, 100, 2, 4, 4, 2, 400, -1, -1)
    assert b"0.2" in capi.lib().moni_version()


def test_cli_extend_option(exe, tmp_path):
    fq = str(tmp_path / "f.fq")
    open(fq, "w").write("@a\nACGTACGT\n+\nIIIIIIII\n")
    out = subprocess.check_output([exe, "x", "-p", fq, "--extend", "--dry-run"]).decode()
    assert "mode=extend" in out and "reads=1 bases=8" in out
    assert "mode=" not in subprocess.check_output([exe, "x", "-p", fq, "--dry-run"]).decode()
    for extra, word in ((["-1", fq, "-2", fq], b"-1 / -2"), (["-p", fq, "-m"], b"-m"), (["-p", fq, "-c"], b"-c"), (["-p", fq, "--ms"], b"--ms"), (["-p", fq, "--mems"], b"--mems")):
        r = subprocess.run([exe, "x", "--extend"] + extra, capture_output=True)
        assert r.returncode == 1 and b"--extend" in r.stderr and word in r.stderr, (extra, r.stderr)
