"""moni-hip-align: which output flag stands beside which mode.  A characterisation of the front end's clash checks, recorded from the binary before those
checks became one table (tests/golden/make_cli_clashes.py wrote tests/golden/cli_clashes.json): every output choice x every mode x single end / pairs,
always under --dry-run, so no GPU is needed.  The binary must answer every cell as it did: exit code, stderr, and for the runs that pass the stdout
(the --dry-run line with its out= name and its bgzf= / bam= / sort= / markdup= words)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "moni_align_amd", "host", "moni-hip-align")
FIXTURE = os.path.join(ROOT, "tests", "golden", "cli_clashes.json")
TMP = "<TMP>"          # stands for the directory of the input files in the recorded text

OUTPUTS = ("--bgzf", "--bam", "--bam --sort", "--bam --sort --mark-dup", "--sort", "--mark-dup", "--bam --bgzf --sort", "--bam --sort-chunk 1000 --sort")
MODES = ("", "-c", "--dry-run-write", "--ms", "--mems", "--pseudo-ms", "--screen", "--locate", "--seq-count", "--loci", "--approx 1", "--extend", "-m")
INPUTS = ("single", "paired")


def cells():
    return [(o, m, i) for o in OUTPUTS for m in MODES for i in INPUTS]


def key(cell):
    return " | ".join(cell)


def write_inputs(d):
    for name, rec in (("x.fq", "@a\nACGT\n+\nIIII\n"), ("x_1.fq", "@a/1\nACGT\n+\nIIII\n"), ("x_2.fq", "@a/2\nTTGA\n+\nIIII\n")):
        with open(os.path.join(d, name), "w") as f:
            f.write(rec)


def answer(exe, d, cell):
    """What the binary says to one cell, the directory of the inputs spelled TMP."""
    out, mode, inp = cell
    reads = ["-p", os.path.join(d, "x.fq")] if inp == "single" else ["-1", os.path.join(d, "x_1.fq"), "-2", os.path.join(d, "x_2.fq")]
    r = subprocess.run([exe, "idx/pref"] + reads + out.split() + mode.split() + ["--dry-run"], capture_output=True, cwd=d)
    got = {"exit": r.returncode, "stderr": r.stderr.decode().replace(d, TMP)}
    if r.returncode == 0:
        got["stdout"] = r.stdout.decode().replace(d, TMP)
    return got


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__
    __graft_entry__.build()
    return EXE


def test_every_cell_answers_as_recorded(exe, tmp_path):
    with open(FIXTURE) as f:
        want = json.load(f)
    assert sorted(want) == sorted(key(c) for c in cells())          # the fixture is the whole cross product
    d = str(tmp_path)
    write_inputs(d)
    wrong = [(key(c), want[key(c)], got) for c in cells() for got in (answer(exe, d, c),) if got != want[key(c)]]
    assert not wrong, "%d of %d cells changed; the first: %r" % (len(wrong), len(want), wrong[0])
    # the recording is not trivially uniform: both outcomes occur, and so does every output word of --dry-run
    assert {v["exit"] for v in want.values()} == {0, 1}
    said = "".join(v.get("stdout", "") for v in want.values())
    for word in (" bgzf=1", " bam=1\n", " bam=1 sort=1\n", " bam=1 sort=1 markdup=1"):
        assert word in said, word
