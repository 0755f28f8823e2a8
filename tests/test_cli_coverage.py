"""`moni-hip-align --bam --sort [--mark-dup] --coverage [--cov-window N] [--cov-mapq Q]`: without a GPU the option parses (--dry-run says
coverage=1 behind sort=1[ markdup=1]), is listed by the usage text, belongs to --sort, refuses the modes that write several records per read,
and changes nothing where it is not given; on the GPU <out>.bam and its index are the bytes of the run without the option, and the three
coverage files are tests/coverage_model applied to the records of the very <out>.bam written - for every batch size and number of contexts."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from tests import bgzf_model as bm
from tests import coverage_model as cm
from tests.test_cli_markdup import EXE, planted, quals


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__
    __graft_entry__.build()
    return EXE


@pytest.fixture(scope="module")
def fq(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("records") / "f.fq")
    open(p, "w").write("@a\nACGTACGT\n+\nIIIIIIII\n@b\nACGT\n+\nIIII\n")
    return p


def test_dry_run_says_coverage(exe, fq):
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "-o", "o.sam", "--bam", "--sort", "--coverage", "--dry-run"]).decode()
    assert out.rstrip().endswith(" bam=1 sort=1 coverage=1") and "Output file: o.bam\n" in out
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "-o", "o.sam", "--bam", "--sort", "--mark-dup", "--coverage", "--cov-window", "500", "--cov-mapq", "20", "--dry-run"]).decode()
    assert out.rstrip().endswith(" bam=1 sort=1 markdup=1 coverage=1")
    out = subprocess.check_output([exe, "idx/pref", "-1", fq, "-2", fq, "-o", "pe.sam", "--coverage", "--mark-dup", "--sort", "--bam", "--dry-run"]).decode()
    assert "pairs=2" in out and out.rstrip().endswith("bam=1 sort=1 markdup=1 coverage=1") and "Output file: pe.bam\n" in out


def test_without_the_option_nothing_changes(exe, fq):
    for args in (["-p", fq, "--bam", "--sort"], ["-p", fq, "--bam", "--sort", "--mark-dup"], ["-p", fq, "--bam"], ["-p", fq], ["-1", fq, "-2", fq, "-o", "pe.sam", "--bam", "--sort"],
                 ["-p", fq, "-o", "o", "--extend", "--bam", "--sort"], ["-p", fq, "--bgzf"]):
        out = subprocess.check_output([exe, "idx/pref"] + args + ["--dry-run"]).decode()
        assert "coverage" not in out
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "--bam", "--sort", "--dry-run"]).decode()
    assert out.rstrip().endswith(" bam=1 sort=1") and ("out=%s_pref_25.bam first=a bam=1 sort=1\n" % fq) in out
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "--bam", "--sort", "--mark-dup", "--dry-run"]).decode()
    assert out.rstrip().endswith("first=a bam=1 sort=1 markdup=1")


@pytest.mark.parametrize("extra,word", [(["--coverage", "--bam"], b"--coverage belongs to --sort"), (["--coverage"], b"--coverage belongs to --sort"),
                                        (["--coverage", "--sort"], b"--sort belongs to --bam"),
                                        (["--coverage", "--bam", "--sort", "--extend"], b"--coverage cannot be combined with --extend"),
                                        (["--coverage", "--bam", "--sort", "-m"], b"--coverage cannot be combined with -m"),
                                        (["--bam", "--sort", "--cov-window", "100"], b"--cov-window belongs to --coverage"),
                                        (["--bam", "--sort", "--cov-mapq", "20"], b"--cov-mapq belongs to --coverage"),
                                        (["--cov-window", "100"], b"--cov-window belongs to --coverage"),
                                        (["--coverage", "--bam", "--sort", "--cov-window", "0"], b"--cov-window takes 1 to 2147483647 bases"),
                                        (["--coverage", "--bam", "--sort", "--cov-window", "2147483648"], b"--cov-window takes 1 to 2147483647 bases"),
                                        (["--coverage", "--bam", "--sort", "--cov-mapq", "256"], b"--cov-mapq takes 0 to 255"),
                                        (["--coverage", "--bam", "--sort", "--gpus", "2"], b"--coverage takes one GPU")])
def test_refuses(exe, fq, tmp_path, extra, word):
    out = str(tmp_path / "o.sam")
    r = subprocess.run([exe, "x", "-p", fq, "-o", out] + extra, capture_output=True)
    assert r.returncode == 1 and word in r.stderr, (extra, r.stderr)
    assert not os.listdir(str(tmp_path))


def test_usage_lists_it(exe):
    r = subprocess.run([exe, "-h"], capture_output=True)
    assert r.returncode == 1 and b"[--mark-dup] [--coverage [--cov-window N] [--cov-mapq Q]]" in r.stderr
    assert b"--coverage: with --sort" in r.stderr and b"--cov-window N:" in r.stderr and b"--cov-mapq Q:" in r.stderr


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------------------

def run(exe, args, out, extra):
    r = subprocess.run([exe] + args + ["-o", out] + extra, capture_output=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


def gunzip_blocks(path):
    z = open(path, "rb").read()
    assert z.endswith(bm.EOF_BLOCK), path
    return gzip.decompress(z)


@pytest.mark.gpu
def test_coverage_files(exe, medium_case, tmp_path):
    """3000 reads and 300 planted copies: two batch sizes, one context and three"""
    reads = medium_case.synth.make_reads(medium_case.pg, 3000, 150, seed=61)
    order = planted(3000, 10, 7)
    rng = np.random.default_rng(11)
    fq = str(tmp_path / "reads.fastq")
    with open(fq, "wb") as f:
        for i, copy in order:
            f.write(b"@%s.%d\n%s\n+\n%s\n" % (b"copy" if copy else b"read", i, reads[i].tobytes(), quals(rng, 150)))
    common = [medium_case.path[:-4], "-p", fq, "-S", "1000", "-F", "0.5", "-t", "4"]
    sort = ["--bam", "--sort", "--sort-chunk", "65536", "--mark-dup"]
    texts = set()
    for k, cfg in enumerate((["--gpu-batch", "250", "--ctx-per-gpu", "3"], ["--gpu-batch", "250", "--ctx-per-gpu", "1"], ["--gpu-batch", "650", "--ctx-per-gpu", "3"])):
        d = str(tmp_path / ("c%d" % k))
        os.mkdir(d)
        plain = run(exe, common + cfg, os.path.join(d, "p.sam"), sort)
        stdout = run(exe, common + cfg, os.path.join(d, "o.sam"), sort + ["--coverage", "--cov-window", "100"])
        assert sorted(os.listdir(d)) == sorted(["p.bam", "p.bam.bai", "o.bam", "o.bam.bai", "o.bam.mosdepth.summary.txt", "o.bam.per-base.bed.gz", "o.bam.regions.bed.gz"])
        assert b"Coverage:" not in plain
        data = open(os.path.join(d, "o.bam"), "rb").read()
        assert data == open(os.path.join(d, "p.bam"), "rb").read(), "configuration %r: --coverage changed the BAM file" % (cfg,)
        assert open(os.path.join(d, "o.bam.bai"), "rb").read() == open(os.path.join(d, "p.bam.bai"), "rb").read()
        m = cm.of_bam_file(data)
        assert m.stats["counted"] > 2000 and m.stats["skipped_flag"] >= 100
        assert open(os.path.join(d, "o.bam.mosdepth.summary.txt"), "rb").read() == m.summary()
        assert gunzip_blocks(os.path.join(d, "o.bam.per-base.bed.gz")) == m.per_base()
        assert gunzip_blocks(os.path.join(d, "o.bam.regions.bed.gz")) == m.regions(100)
        line = ("Coverage: %d counted of %d records, mean depth %.2f" % (m.stats["counted"], m.stats["records"], m.mean_depth())).encode()
        assert line in stdout, (line, re.findall(rb"Coverage:[^\n]*", stdout))
        # the duplicates that were marked do not count: a run that ignored 0x400 would give this text
        assert cm.of_bam_file(data, exclude=0x304).per_base() != m.per_base()
        texts.add(m.per_base())
    assert len(texts) == 1, "the depth depends on the batches"


@pytest.mark.gpu
def test_mapq_threshold_and_no_window(exe, medium_case, tmp_path):
    reads = medium_case.synth.make_reads(medium_case.pg, 600, 150, seed=62)
    fq = str(tmp_path / "reads.fastq")
    with open(fq, "wb") as f:
        for i in range(len(reads)):
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, reads[i].tobytes(), b"I" * 150))
    d = str(tmp_path / "q")
    os.mkdir(d)
    run(exe, [medium_case.path[:-4], "-p", fq, "-S", "1000", "-F", "0.5", "-t", "2"], os.path.join(d, "o.sam"), ["--bam", "--sort", "--coverage", "--cov-mapq", "30"])
    assert sorted(os.listdir(d)) == ["o.bam", "o.bam.bai", "o.bam.mosdepth.summary.txt", "o.bam.per-base.bed.gz"]
    data = open(os.path.join(d, "o.bam"), "rb").read()
    m = cm.of_bam_file(data, min_mapq=30)
    assert gunzip_blocks(os.path.join(d, "o.bam.per-base.bed.gz")) == m.per_base()
    assert open(os.path.join(d, "o.bam.mosdepth.summary.txt"), "rb").read() == m.summary()
