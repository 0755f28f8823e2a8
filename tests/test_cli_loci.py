"""`moni-hip-align --loci`: the option parses (--dry-run), names its output as the legacy modes do and refuses the inputs and modes it cannot be
combined with (no GPU needed); under -m gpu the `.loci` file equals, byte for byte, the lines formatted from brute force on the same patterns."""
import os
import subprocess

import pytest

from tests import locate_model as lm
from tests import loci_model as lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "moni_align_amd", "host", "moni-hip-align")


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__
    __graft_entry__.build()
    return EXE


@pytest.fixture(scope="module")
def fq(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("loci") / "f.fq")
    open(p, "w").write("@a\nACGTACGT\n+\nIIIIIIII\n@b\nACGT\n+\nIIII\n")
    return p


def test_dry_run_parses(exe, fq):
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "--loci", "--dry-run"]).decode()
    assert "mode=loci strands=1" in out and "reads=2 bases=12" in out
    assert "Output file: %s_pref\n" % fq in out          # <patterns>_<index basename>; the mode appends .loci
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "-o", "o", "--loci", "--both-strands", "--max-walk", "7", "--no-lift", "--dry-run"]).decode()
    assert "mode=loci strands=2" in out and "Output file: o\n" in out


@pytest.mark.parametrize("extra,word", [(["-1", "F", "-2", "F"], b"-1 / -2"), (["-p", "F", "--ms"], b"--ms"), (["-p", "F", "--mems"], b"--mems"),
                                        (["-p", "F", "--extend"], b"--extend"), (["-p", "F", "--pseudo-ms"], b"--pseudo-ms"), (["-p", "F", "-m"], b"with -m\n"),
                                        (["-p", "F", "-c"], b"with -c\n"), (["-p", "F", "--locate"], b"--locate"), (["-p", "F", "--seq-count"], b"--seq-count"),
                                        (["-p", "F", "--approx", "1"], b"--approx")])
def test_refuses_clashes(exe, fq, extra, word):
    r = subprocess.run([exe, "x", "--loci"] + [fq if x == "F" else x for x in extra], capture_output=True)
    assert r.returncode == 1 and b"--loci" in r.stderr and word in r.stderr, (extra, r.stderr)


def test_refuses_its_option_without_the_mode_and_lists_itself(exe, fq):
    r = subprocess.run([exe, "x", "-p", fq, "--no-lift"], capture_output=True)
    assert r.returncode == 1 and b"--no-lift belongs to --loci" in r.stderr
    r = subprocess.run([exe, "x", "-p", fq, "--seq-count", "--no-lift"], capture_output=True)
    assert r.returncode == 1 and b"--no-lift belongs to --loci" in r.stderr
    r = subprocess.run([exe, "x", "-p", fq, "--max-walk", "3"], capture_output=True)
    assert r.returncode == 1 and b"--loci" in r.stderr
    r = subprocess.run([exe, "-h"], capture_output=True)
    assert r.returncode == 1 and b"--loci [--max-walk N] [--both-strands] [--no-lift]" in r.stderr


def lines(names, seq_names, text, pats, seq_starts, strands, max_walk, keymap):
    """the file, from brute force alone"""
    import numpy as np
    starts = np.asarray(seq_starts).astype(np.int64)
    out = []
    for nm, p in zip(names, pats):
        for s in range(strands):
            count, matched, loci = lo.brute_loci(text, lm.revcomp(p) if s else p, keymap)
            if max_walk and count > max_walk:
                n, lst = 0, "?"
            else:
                sq = np.searchsorted(starts, [k for k, _ in loci], side="right") - 1
                n = len(loci)
                lst = ",".join("%s:%d:%d" % (seq_names[q], k - int(starts[q]) + 1, v) for q, (k, v) in zip(sq, loci)) or "*"
            out.append("%s\t%s\t%d\t%d\t%d\t%s\n" % (nm, "-" if s else "+", count, matched, n, lst))
    return "".join(out).encode()


@pytest.mark.gpu
@pytest.mark.parametrize("flags,strands,max_walk,lift,fasta", [(["--max-walk", "800", "--both-strands"], 2, 800, 1, False), (["--no-lift"], 1, 1 << 20, 0, True),
                                                               (["--no-lift", "--both-strands", "--max-walk", "0"], 2, 0, 0, False), ([], 1, 1 << 20, 1, True)])
def test_file_equals_brute_force(exe, tmp_path, flags, strands, max_walk, lift, fasta):
    pg, fi, text, pats = lo.lifted_case()
    pats = [p for p in pats if p]                            # what a FASTA / FASTQ record can carry
    names = ["pat%d" % i for i in range(len(pats))]
    path = str(tmp_path / "lifted.mfi")
    fi.save(path)
    src = str(tmp_path / ("p.fa" if fasta else "p.fq"))
    with open(src, "wb") as f:
        for nm, p in zip(names, pats):
            f.write((b">%s\n%s\n" if fasta else b"@%s some comment\n%s\n+\n" + b"I" * len(p) + b"\n") % (nm.encode(), p))
    out = str(tmp_path / "res")
    r = subprocess.run([exe, path[:-4], "-p", src, "-o", out, "--loci", "--gpu-batch", "7", "-t", "2"] + flags, capture_output=True)          # several batches in flight
    assert r.returncode == 0, r.stderr
    got = open(out + ".loci", "rb").read()
    assert got == lines(names, fi.names, text, pats, fi.seq_starts, strands, max_walk, lo.text_to_ref(pg) if lift else None)
    assert got.count(b"\n") == len(pats) * strands and (b"\t?\n" in got) == (max_walk == 800)
    first = got.split(b"\n")[0].split(b"\t")                 # the pattern A
    if max_walk != 800:
        assert first[:5] == [b"pat0", b"+", b"9125", b"1", b"1527" if lift else b"9125"]
        assert (b":8," in first[5]) == bool(lift) and first[5].startswith(b"chr19:")
    if lift:
        assert b"S1_H1_chr19:" not in got                    # every locus is on the reference contig
