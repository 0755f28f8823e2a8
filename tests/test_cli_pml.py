"""`moni-hip-align --pseudo-ms` without a GPU: the option parses (--dry-run), names its output as the other legacy modes do, and refuses the
inputs and modes it cannot be combined with."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "moni_align_amd", "host", "moni-hip-align")


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__
    __graft_entry__.build()
    return EXE


@pytest.fixture(scope="module")
def fq(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("pml") / "f.fq")
    open(p, "w").write("@a\nACGTACGT\n+\nIIIIIIII\n@b\nACGT\n+\nIIII\n")
    return p


def test_dry_run_parses(exe, fq):
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "--pseudo-ms", "--dry-run"]).decode()
    assert "mode=pseudo-ms" in out and "reads=2 bases=12" in out
    assert "Output file: %s_pref\n" % fq in out          # <patterns>_<index basename>; the mode appends .pseudo_lengths
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "-o", "o", "-l", "30", "--pseudo-ms", "--dry-run"]).decode()
    assert "mode=pseudo-ms" in out and "Output file: o\n" in out and "min_len=30" in out
    assert "mode=" not in subprocess.check_output([exe, "idx/pref", "-p", fq, "--dry-run"]).decode()


@pytest.mark.parametrize("extra,word", [(["-1", "F", "-2", "F"], b"-1 / -2"), (["-p", "F", "--ms"], b"--ms"), (["-p", "F", "--mems"], b"--mems"),
                                        (["-p", "F", "--extend"], b"--extend"), (["-p", "F", "-m"], b"with -m\n"), (["-p", "F", "-c"], b"with -c\n")])
def test_refuses_clashes(exe, fq, extra, word):
    r = subprocess.run([exe, "x", "--pseudo-ms"] + [fq if x == "F" else x for x in extra], capture_output=True)
    assert r.returncode == 1 and b"--pseudo-ms" in r.stderr and word in r.stderr, (extra, r.stderr)


def test_usage_lists_it(exe):
    r = subprocess.run([exe, "-h"], capture_output=True)
    assert r.returncode == 1 and b"--pseudo-ms" in r.stderr
