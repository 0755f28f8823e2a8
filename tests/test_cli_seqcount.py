"""`moni-hip-align --seq-count`: the option parses (--dry-run), names its output as the legacy modes do and refuses the inputs and modes it cannot
be combined with (no GPU needed); under -m gpu the `.seqcount` file equals the lines formatted from brute force on the same patterns."""
import os
import subprocess

import pytest

from tests import locate_model as lm
from tests import seqcount_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "moni_align_amd", "host", "moni-hip-align")


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__
    __graft_entry__.build()
    return EXE


@pytest.fixture(scope="module")
def fq(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("sc") / "f.fq")
    open(p, "w").write("@a\nACGTACGT\n+\nIIIIIIII\n@b\nACGT\n+\nIIII\n")
    return p


def test_dry_run_parses(exe, fq):
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "--seq-count", "--dry-run"]).decode()
    assert "mode=seq-count strands=1" in out and "reads=2 bases=12" in out
    assert "Output file: %s_pref\n" % fq in out          # <patterns>_<index basename>; the mode appends .seqcount
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "-o", "o", "--seq-count", "--both-strands", "--max-walk", "7", "--dry-run"]).decode()
    assert "mode=seq-count strands=2" in out and "Output file: o\n" in out


@pytest.mark.parametrize("extra,word", [(["-1", "F", "-2", "F"], b"-1 / -2"), (["-p", "F", "--ms"], b"--ms"), (["-p", "F", "--mems"], b"--mems"),
                                        (["-p", "F", "--extend"], b"--extend"), (["-p", "F", "--pseudo-ms"], b"--pseudo-ms"), (["-p", "F", "-m"], b"with -m\n"),
                                        (["-p", "F", "-c"], b"with -c\n"), (["-p", "F", "--locate"], b"--locate")])
def test_refuses_clashes(exe, fq, extra, word):
    r = subprocess.run([exe, "x", "--seq-count"] + [fq if x == "F" else x for x in extra], capture_output=True)
    assert r.returncode == 1 and b"--seq-count" in r.stderr and word in r.stderr, (extra, r.stderr)


def test_refuses_its_option_without_the_mode_and_lists_itself(exe, fq):
    r = subprocess.run([exe, "x", "-p", fq, "--max-walk", "3"], capture_output=True)
    assert r.returncode == 1 and b"--seq-count" in r.stderr
    r = subprocess.run([exe, "-h"], capture_output=True)
    assert r.returncode == 1 and b"--seq-count [--max-walk N] [--both-strands]" in r.stderr


def lines(names, seq_names, text, pats, seq_starts, strands, max_walk):
    """the file, from brute force alone"""
    out = []
    for nm, p in zip(names, pats):
        for s in range(strands):
            count, matched, row = sm.brute_row(text, lm.revcomp(p) if s else p, seq_starts)
            if max_walk and count > max_walk:
                n_seqs, lst = 0, "?"
            else:
                n_seqs = int((row != 0).sum())
                lst = ",".join("%s:%d" % (seq_names[q], int(v)) for q, v in enumerate(row) if v) or "*"
            out.append("%s\t%s\t%d\t%d\t%d\t%s\n" % (nm, "-" if s else "+", count, matched, n_seqs, lst))
    return "".join(out).encode()


@pytest.mark.gpu
@pytest.mark.parametrize("flags,strands,max_walk,fasta", [(["--max-walk", "8", "--both-strands"], 2, 8, False), ([], 1, 1 << 20, True)])
def test_file_equals_brute_force(exe, tmp_path, flags, strands, max_walk, fasta):
    fi, text, pats = lm.planted_case()
    every = len(pats)
    pats = [p for p in pats if p and all(65 <= b < 123 for b in p)]          # what a FASTA / FASTQ record can carry
    assert len(pats) == every - 6 and pats[19] == lm.planted_case()[2][19] and b"NNNN" in pats and b"acgt" in pats and b"X" in pats
    names = ["pat%d" % i for i in range(len(pats))]
    path = str(tmp_path / "planted.mfi")
    fi.save(path)
    src = str(tmp_path / ("p.fa" if fasta else "p.fq"))
    with open(src, "wb") as f:
        for nm, p in zip(names, pats):
            f.write((b">%s\n%s\n" if fasta else b"@%s some comment\n%s\n+\n" + b"I" * len(p) + b"\n") % (nm.encode(), p))
    out = str(tmp_path / "res")
    r = subprocess.run([exe, path[:-4], "-p", src, "-o", out, "--seq-count", "--gpu-batch", "7", "-t", "2"] + flags, capture_output=True)          # several batches in flight
    assert r.returncode == 0, r.stderr
    got = open(out + ".seqcount", "rb").read()
    assert got == lines(names, fi.names, text, pats, fi.seq_starts, strands, max_walk)
    assert got.count(b"\n") == len(pats) * strands and b"ref:" in got and b"\t*\n" in got and (b"\t?\n" in got) == (max_walk == 8)
