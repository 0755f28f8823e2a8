"""`moni-hip-align --locate`: the option parses (--dry-run), names its output as the legacy modes do and refuses the inputs and modes it cannot be
combined with (no GPU needed); under -m gpu the `.locate` file equals the lines made from the library call on the same patterns."""
import os
import subprocess

import numpy as np
import pytest

from tests import locate_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "moni_align_amd", "host", "moni-hip-align")


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__
    __graft_entry__.build()
    return EXE


@pytest.fixture(scope="module")
def fq(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("loc") / "f.fq")
    open(p, "w").write("@a\nACGTACGT\n+\nIIIIIIII\n@b\nACGT\n+\nIIII\n")
    return p


def test_dry_run_parses(exe, fq):
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "--locate", "--dry-run"]).decode()
    assert "mode=locate strands=1" in out and "reads=2 bases=12" in out
    assert "Output file: %s_pref\n" % fq in out          # <patterns>_<index basename>; the mode appends .locate
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "-o", "o", "--locate", "--both-strands", "--max-occ", "7", "--dry-run"]).decode()
    assert "mode=locate strands=2" in out and "Output file: o\n" in out
    assert "mode=" not in subprocess.check_output([exe, "idx/pref", "-p", fq, "--dry-run"]).decode()


@pytest.mark.parametrize("extra,word", [(["-1", "F", "-2", "F"], b"-1 / -2"), (["-p", "F", "--ms"], b"--ms"), (["-p", "F", "--mems"], b"--mems"),
                                        (["-p", "F", "--extend"], b"--extend"), (["-p", "F", "--pseudo-ms"], b"--pseudo-ms"), (["-p", "F", "-m"], b"with -m\n"),
                                        (["-p", "F", "-c"], b"with -c\n")])
def test_refuses_clashes(exe, fq, extra, word):
    r = subprocess.run([exe, "x", "--locate"] + [fq if x == "F" else x for x in extra], capture_output=True)
    assert r.returncode == 1 and b"--locate" in r.stderr and word in r.stderr, (extra, r.stderr)


def test_refuses_its_options_without_the_mode(exe, fq):
    for extra in (["--max-occ", "3"], ["--both-strands"]):
        r = subprocess.run([exe, "x", "-p", fq] + extra, capture_output=True)
        assert r.returncode == 1 and b"--locate" in r.stderr


def test_usage_lists_it(exe):
    r = subprocess.run([exe, "-h"], capture_output=True)
    assert r.returncode == 1 and b"--locate [--max-occ N] [--both-strands]" in r.stderr


def lines(names, seq_names, res, sq, so, strands):
    out = []
    for i, nm in enumerate(names):
        for s in range(strands):
            r = res[i * strands + s]
            o, k = int(r["occ_off"]), int(r["n_occ"])
            occ = ",".join("%s:%d" % (seq_names[int(sq[o + j])], int(so[o + j]) + 1) for j in range(k)) if k else "*"
            out.append("%s\t%s\t%d\t%d\t%s\n" % (nm, "-" if s else "+", int(r["count"]), int(r["matched"]), occ))
    return "".join(out).encode()


@pytest.mark.gpu
@pytest.mark.parametrize("flags,strands,max_occ,fasta", [(["--max-occ", "4", "--both-strands"], 2, 4, False), ([], 1, 0, True)])
def test_file_equals_the_library_call(exe, tmp_path, flags, strands, max_occ, fasta):
    from moni_align_amd import capi
    fi, text, pats = lm.planted_case()
    every = len(pats)
    pats = [p for p in pats if p and all(65 <= b < 123 for b in p)]          # what a FASTA / FASTQ record can carry
    # left out: the empty pattern and the five with a terminator or separator byte; kept: the planted unit, N, lower case, absent bytes, dying patterns
    assert len(pats) == every - 6 and pats[19] == lm.planted_case()[2][19] and b"NNNN" in pats and b"acgt" in pats and b"X" in pats
    names = ["pat%d" % i for i in range(len(pats))]
    path = str(tmp_path / "planted.mfi")
    fi.save(path)
    src = str(tmp_path / ("p.fa" if fasta else "p.fq"))
    with open(src, "wb") as f:
        for nm, p in zip(names, pats):
            f.write((b">%s\n%s\n" if fasta else b"@%s some comment\n%s\n+\n" + b"I" * len(p) + b"\n") % (nm.encode(), p))
    out = str(tmp_path / "res")
    r = subprocess.run([exe, path[:-4], "-p", src, "-o", out, "--locate", "--gpu-batch", "20", "-t", "2"] + flags, capture_output=True)
    assert r.returncode == 0, r.stderr
    idx = capi.Index(fi=fi, device=0)
    ctx = capi.Ctx(idx)
    try:
        res, pos, sq, so = ctx.locate_batch(*lm.ragged(pats), strands=strands, max_occ=max_occ)
    finally:
        ctx.close()
        idx.close()
    lm.check_against_brute(text, pats, res, pos, sq, so, strands, max_occ, fi.seq_starts)
    got = open(out + ".locate", "rb").read()
    assert got == lines(names, fi.names, res, sq, so, strands)
    assert got.count(b"\n") == len(pats) * strands and (b"ref:" in got) == (max_occ > 0) and b"\t*\n" in got
