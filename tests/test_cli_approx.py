"""`moni-hip-align --approx K`: the option parses (--dry-run), names its output as the other query modes do, refuses the inputs and modes it cannot be
combined with and its own options without it (no GPU needed); under -m gpu the `.approx` file equals the lines formatted from brute force on the
same patterns."""
import os
import subprocess

import pytest

from tests import approx_model as am
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
    p = str(tmp_path_factory.mktemp("apx") / "f.fq")
    open(p, "w").write("@a\nACGTACGT\n+\nIIIIIIII\n@b\nACGT\n+\nIIII\n")
    return p


def test_dry_run_parses(exe, fq):
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "--approx", "2", "--dry-run"]).decode()
    assert "mode=approx k=2 strands=1" in out and "reads=2 bases=12" in out
    assert "Output file: %s_pref\n" % fq in out          # <patterns>_<index basename>; the mode appends .approx
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "-o", "o", "--approx", "0", "--both-strands", "--max-hits", "3", "--max-occ", "2", "--max-steps", "100",
                                   "--dry-run"]).decode()
    assert "mode=approx k=0 strands=2" in out and "Output file: o\n" in out


@pytest.mark.parametrize("extra,word", [(["-1", "F", "-2", "F"], b"-1 / -2"), (["-p", "F", "--ms"], b"--ms"), (["-p", "F", "--mems"], b"--mems"),
                                        (["-p", "F", "--extend"], b"--extend"), (["-p", "F", "--pseudo-ms"], b"--pseudo-ms"), (["-p", "F", "-m"], b"with -m\n"),
                                        (["-p", "F", "-c"], b"with -c\n"), (["-p", "F", "--locate"], b"--locate"), (["-p", "F", "--seq-count"], b"--seq-count")])
def test_refuses_clashes(exe, fq, extra, word):
    r = subprocess.run([exe, "x", "--approx", "1"] + [fq if x == "F" else x for x in extra], capture_output=True)
    assert r.returncode == 1 and b"--approx" in r.stderr and word in r.stderr, (extra, r.stderr)


def test_refuses_bad_values(exe, fq):
    r = subprocess.run([exe, "x", "-p", fq, "--approx", "4"], capture_output=True)
    assert r.returncode == 1 and b"--approx" in r.stderr and b"0 to 3" in r.stderr
    r = subprocess.run([exe, "x", "-p", fq, "--approx", "1", "--max-hits", "0", "--max-occ", "2"], capture_output=True)
    assert r.returncode == 1 and b"--approx" in r.stderr and b"--max-hits" in r.stderr


def test_refuses_its_options_without_the_mode_and_lists_itself(exe, fq):
    for opt in ("--max-hits", "--max-steps"):
        r = subprocess.run([exe, "x", "-p", fq, opt, "3"], capture_output=True)
        assert r.returncode == 1 and b"--approx" in r.stderr, opt
    r = subprocess.run([exe, "x", "-p", fq, "--max-occ", "3"], capture_output=True)          # the options it shares still name --locate without a mode
    assert r.returncode == 1 and b"--locate" in r.stderr
    r = subprocess.run([exe, "x", "-p", fq, "--both-strands"], capture_output=True)
    assert r.returncode == 1 and b"--locate" in r.stderr
    r = subprocess.run([exe, "-h"], capture_output=True)
    assert r.returncode == 1 and b"--approx K [--max-hits N] [--max-occ N] [--both-strands] [--max-steps N]" in r.stderr
    assert b"--locate [--max-occ N] [--both-strands]" in r.stderr and b"--seq-count [--max-walk N] [--both-strands]" in r.stderr


def lines(names, seq_names, text, pats, seq_starts, strands, k, max_occ):
    """the file, from brute force alone (every hit kept)"""
    out = []
    for nm, p in zip(names, pats):
        for s in range(strands):
            cnt, hits = am.brute_task(text, lm.revcomp(p) if s else p, k, max_occ, seq_starts)
            lst = ";".join("%d:%d:%s" % (d, count, ",".join("%s:%d" % (seq_names[q], o + 1) for q, o in zip(sq, so)) or "*") for d, _, count, _, sq, so in hits) or "*"
            out.append("%s\t%s\t1\t%s\t%d\t%s\n" % (nm, "-" if s else "+", ",".join(str(c) for c in cnt[:k + 1]), len(hits), lst))
    return "".join(out).encode()


@pytest.mark.gpu
def test_file_equals_brute_force(exe, tmp_path):
    fi, text, pats = lm.planted_case()
    every = len(pats)
    pats = [p for p in pats if p and all(65 <= b < 123 for b in p)]          # what a FASTA / FASTQ record can carry
    assert len(pats) == every - 6 and b"NNNN" in pats and b"acgt" in pats and b"X" in pats
    names = ["pat%d" % i for i in range(len(pats))]
    want = lines(names, fi.names, text, pats, fi.seq_starts, 2, 2, 3)
    most = max(int(ln.split(b"\t")[4]) for ln in want.splitlines())
    path = str(tmp_path / "planted.mfi")
    fi.save(path)
    src = str(tmp_path / "p.fq")
    with open(src, "wb") as f:
        for nm, p in zip(names, pats):
            f.write(b"@%s some comment\n%s\n+\n" % (nm.encode(), p) + b"I" * len(p) + b"\n")
    out = str(tmp_path / "res")
    r = subprocess.run([exe, path[:-4], "-p", src, "-o", out, "--approx", "2", "--both-strands", "--max-occ", "3", "--max-hits", str(most + 1), "--gpu-batch", "7", "-t", "2"],
                       capture_output=True)          # several batches in flight
    assert r.returncode == 0, r.stderr
    got = open(out + ".approx", "rb").read()
    assert got == want
    assert got.count(b"\n") == len(pats) * 2 and b"ref:" in got and b"\t*\n" in got and b";1:" in got and b";2:" in got
