"""`moni-hip-align --screen`: without a GPU the option parses (--dry-run), names its output as the other pattern modes do and refuses what it
cannot be combined with; on the GPU <out>.screen equals the text of tests/screen_model.render, in input order across batches."""
import os
import subprocess

import numpy as np
import pytest

from tests import pml_model, screen_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "moni_align_amd", "host", "moni-hip-align")


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__
    __graft_entry__.build()
    return EXE


@pytest.fixture(scope="module")
def fq(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("screen") / "f.fq")
    open(p, "w").write("@a\nACGTACGT\n+\nIIIIIIII\n@b\nACGT\n+\nIIII\n")
    return p


def test_dry_run_parses(exe, fq):
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "--screen", "--dry-run"]).decode()
    assert "mode=screen strands=2" in out and "reads=2 bases=12" in out
    assert "Output file: %s_pref\n" % fq in out          # <patterns>_<index basename>; the mode appends .screen
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "-o", "o", "--screen", "--window", "64", "--min-win", "32", "--ks", "1/2", "--one-strand", "--dry-run"]).decode()
    assert "mode=screen strands=1" in out and "Output file: o\n" in out


@pytest.mark.parametrize("extra,word", [(["-1", "F", "-2", "F"], b"-1 / -2"), (["-p", "F", "--ms"], b"--ms"), (["-p", "F", "--mems"], b"--mems"),
                                        (["-p", "F", "--extend"], b"--extend"), (["-p", "F", "--pseudo-ms"], b"--pseudo-ms"), (["-p", "F", "--locate"], b"--locate"),
                                        (["-p", "F", "--seq-count"], b"--seq-count"), (["-p", "F", "--loci"], b"--loci"), (["-p", "F", "--approx", "1"], b"--approx"),
                                        (["-p", "F", "-m"], b"with -m\n"), (["-p", "F", "-c"], b"with -c\n")])
def test_refuses_clashes(exe, fq, extra, word):
    r = subprocess.run([exe, "x", "--screen"] + [fq if x == "F" else x for x in extra], capture_output=True)
    assert r.returncode == 1 and b"--screen" in r.stderr and word in r.stderr, (extra, r.stderr)


@pytest.mark.parametrize("opt,word", [(["--window", "7"], b"--window takes"), (["--window", "65536"], b"--window takes"), (["--min-win", "51"], b"--min-win takes"),
                                      (["--min-win", "0"], b"--min-win takes"), (["--ks", "3/2"], b"--ks takes"), (["--ks", "1"], b"--ks takes"), (["--ks", "0/4"], b"--ks takes")])
def test_refuses_parameters_out_of_range(exe, fq, opt, word):
    r = subprocess.run([exe, "x", "-p", fq, "--screen"] + opt, capture_output=True)
    assert r.returncode == 1 and word in r.stderr, (opt, r.stderr)


def test_options_belong_to_the_mode(exe, fq):
    for opt in (["--window", "64"], ["--min-win", "10"], ["--ks", "1/2"], ["--one-strand"]):
        r = subprocess.run([exe, "x", "-p", fq] + opt, capture_output=True)
        assert r.returncode == 1 and b"belong to --screen" in r.stderr, (opt, r.stderr)


def test_usage_lists_it(exe):
    r = subprocess.run([exe, "-h"], capture_output=True)
    assert r.returncode == 1 and b"--screen [--window N] [--min-win N] [--ks NUM/DEN] [--one-strand]" in r.stderr


def mixed_reads(case, n):
    """simulated 75-base reads (two scored windows: 50 and 25 offsets) with every fifth one random"""
    reads = case.synth.make_reads(case.pg, n, 75, seed=91, sub_rate=0.02, indel_rate=0.003)
    rng = np.random.default_rng(92)
    reads[::5] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=reads[::5].shape)]
    return reads


@pytest.fixture(scope="module")
def screened(medium_case):
    """2500 reads and the model's walks of them, shared by the runs below"""
    reads = mixed_reads(medium_case, 2500)
    model = pml_model.PmlModel(medium_case.fi)
    rb = [x.tobytes() for x in reads]
    return reads, rb, model, [sm.walk_read(model, r) for r in rb]


@pytest.mark.gpu
def test_fastq_across_batches(exe, medium_case, screened, tmp_path):
    reads, rb, model, walked = screened
    fq = str(tmp_path / "reads.fastq")
    medium_case.synth.write_fastq(fq, reads)
    out = str(tmp_path / "scr")
    r = subprocess.run([exe, medium_case.path[:-4], "-p", fq, "-o", out, "--screen", "--gpu-batch", "900", "-t", "4"], capture_output=True)
    assert r.returncode == 0, r.stderr
    recs = [sm.screen_read(model, x, walked=w) for x, w in zip(rb, walked)]
    names = [b"simulated.%d" % i for i in range(len(rb))]
    want = sm.render(names, rb, recs)
    got = open(out + ".screen", "rb").read()
    assert got == want
    assert b"\nsimulated.899\t" in got and b"\nsimulated.900\t" in got and b"\nsimulated.2499\t" in got          # the names cross the batches' borders
    n_p = sm.n_present(recs)
    assert b"Number of reads called present: %d/2500" % n_p in r.stdout + r.stderr
    assert got.count(b"\tP\t-\t") > 500 and got.count(b"\tP\t+\t") > 500 and got.count(b"\tA\t.\t") >= 450          # every fifth read is random


@pytest.mark.gpu
def test_fasta_one_strand_and_parameters(exe, medium_case, screened, tmp_path):
    reads, rb, model, walked = screened
    rb, walked = rb[:300], walked[:300]
    fa = str(tmp_path / "reads.fa")
    with open(fa, "wb") as f:
        for i, x in enumerate(rb):
            f.write(b">q%d\n" % i + x + b"\n")
    names = [b"q%d" % i for i in range(len(rb))]
    for opts, p in ((["--one-strand"], sm.Params(strands=1)), (["--window", "64", "--min-win", "32", "--ks", "1/2"], sm.Params(64, 32, 1, 2))):
        out = str(tmp_path / "scr_fa")
        r = subprocess.run([exe, medium_case.path[:-4], "-p", fa, "-o", out, "--screen", "--gpu-batch", "128"] + opts, capture_output=True)
        assert r.returncode == 0, r.stderr
        want = sm.render(names, rb, [sm.screen_read(model, x, p, walked=w) for x, w in zip(rb, walked)])
        assert open(out + ".screen", "rb").read() == want
    assert b"\t-\t" not in sm.render(names, rb, [sm.screen_read(model, x, sm.Params(strands=1), walked=w) for x, w in zip(rb, walked)])


@pytest.mark.gpu
def test_conflicting_mode_exits_nonzero(exe, medium_case, tmp_path):
    fq = str(tmp_path / "r.fastq")
    medium_case.synth.write_fastq(fq, mixed_reads(medium_case, 4))
    r = subprocess.run([exe, medium_case.path[:-4], "-p", fq, "-o", str(tmp_path / "x"), "--screen", "--pseudo-ms"], capture_output=True)
    assert r.returncode != 0 and b"--screen cannot be combined with --pseudo-ms" in r.stderr
    assert not os.path.exists(str(tmp_path / "x.screen"))
