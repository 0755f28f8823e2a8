"""`moni-hip-align --bam`: without a GPU the option parses (--dry-run), names its output, is listed by the usage text and refuses --bgzf and
the modes that write no SAM; on the GPU <out>.bam is a BGZF file (tests/bgzf_model.walk) that ends with the end-of-file block and whose
content, read by the strict reader of tests/bam_model.py, is the plain run's SAM file - header included - in every SAM mode and with several
batches and contexts in flight."""
import gzip
import os
import subprocess

import pytest

from tests import bam_model as bam
from tests import bgzf_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "moni_align_amd", "host", "moni-hip-align")


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__
    __graft_entry__.build()
    return EXE


@pytest.fixture(scope="module")
def fq(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("records") / "f.fq")          # (a name without the option's: the tests look for it in the output)
    open(p, "w").write("@a\nACGTACGT\n+\nIIIIIIII\n@b\nACGT\n+\nIIII\n")
    return p


def test_dry_run_parses_and_names(exe, fq):
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "--bam", "--dry-run"]).decode()
    assert " bam=1" in out and "reads=2 bases=12" in out
    assert "Output file: %s_pref_25.bam\n" % fq in out and "out=%s_pref_25.bam " % fq in out          # the default name's .sam becomes .bam
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "-o", "o.sam", "--bam", "--extend", "--gpus", "2", "--ctx-per-gpu", "2", "--dry-run"]).decode()
    assert " bam=1" in out and "mode=extend" in out and "Output file: o.bam\n" in out and "gpus=2" in out
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "-o", "o.txt", "-m", "--bam", "--dry-run"]).decode()
    assert " bam=1" in out and "Output file: o.txt.bam\n" in out                                       # any other name gets .bam appended
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "-o", "sam", "--bam", "--dry-run"]).decode()
    assert "Output file: sam.bam\n" in out
    out = subprocess.check_output([exe, "idx/pref", "-1", fq, "-2", fq, "-o", "pe.sam", "--bam", "--dry-run"]).decode()
    assert "pairs=2" in out and out.rstrip().endswith("bam=1") and "Output file: pe.bam\n" in out and "out=pe.bam " in out
    out = subprocess.check_output([exe, "idx/pref", "-1", fq, "-2", fq, "--bam", "--dry-run"]).decode()
    assert "Output file: %s_pref_25.bam\n" % fq in out


def test_without_the_option_nothing_changes(exe, fq):
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "--dry-run"]).decode()
    assert "bam" not in out and "Output file: %s_pref_25.sam\n" % fq in out and ("out=%s_pref_25.sam first=a\n" % fq) in out
    out = subprocess.check_output([exe, "idx/pref", "-1", fq, "-2", fq, "-o", "pe.sam", "--dry-run"]).decode()
    assert "bam" not in out and "out=pe.sam first=a second=a\n" in out
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "-o", "o", "--extend", "--dry-run"]).decode()
    assert "bam" not in out and out.rstrip().endswith("mode=extend") and "Output file: o\n" in out
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "-o", "o.sam", "--bgzf", "--dry-run"]).decode()
    assert "bam" not in out and out.rstrip().endswith("bgzf=1") and "Output file: o.sam.gz\n" in out


@pytest.mark.parametrize("extra,word", [(["--bgzf"], b"with --bgzf\n"), (["-c"], b"with -c\n"), (["--dry-run-write"], b"--dry-run-write"), (["--ms"], b"--ms"),
                                        (["--mems"], b"--mems"), (["--pseudo-ms"], b"--pseudo-ms"), (["--screen"], b"--screen"), (["--locate"], b"--locate"),
                                        (["--seq-count"], b"--seq-count"), (["--loci"], b"--loci"), (["--approx", "1"], b"--approx")])
def test_refuses_clashes(exe, fq, tmp_path, extra, word):
    out = str(tmp_path / "o.sam")
    r = subprocess.run([exe, "x", "-p", fq, "-o", out, "--bam"] + extra, capture_output=True)
    assert r.returncode == 1 and b"--bam cannot be combined with " in r.stderr and word in r.stderr, (extra, r.stderr)
    assert not os.listdir(str(tmp_path))
    if extra in (["-c"], ["--bgzf"]):
        r = subprocess.run([exe, "x", "-1", fq, "-2", fq, "-o", out, "--bam"] + extra, capture_output=True)
        assert r.returncode == 1 and b"--bam cannot be combined with " + extra[0].encode() in r.stderr


def test_usage_lists_it(exe):
    r = subprocess.run([exe, "-h"], capture_output=True)
    assert r.returncode == 1 and b"[--bgzf] [--bam]" in r.stderr and b"--bam: the SAM output" in r.stderr


def both_ways(exe, args, out):
    """the run with and without --bam; returns (the plain file, the blocks of the .bam file)"""
    for extra in ([], ["--bam"]):
        r = subprocess.run([exe] + args + ["-o", out] + extra, capture_output=True)
        assert r.returncode == 0, r.stderr
    plain = open(out, "rb").read()
    assert out.endswith(".sam") and not os.path.exists(out + ".bam")
    z = open(out[:-4] + ".bam", "rb").read()
    blocks = bm.walk(z)
    assert z.endswith(bm.EOF_BLOCK) and blocks[-1] == (b"", 1) and all(len(b) > 0 for b, _ in blocks[:-1])
    stream = gzip.decompress(z)
    assert stream == b"".join(b for b, _ in blocks)
    # the strict reader gives the plain run's file, as far as a BAM carries it (tests/bam_model.canonical: the case of a base, `=` beside `*`)
    assert bam.decode(stream) == bam.canonical(plain)
    header, lines = bam.split_sam(plain)
    assert plain.startswith(b"@HD") and stream == bam.encode(header, lines)
    assert blocks[0][0] == bam.encode_header(header), "the header is in blocks of its own"
    return plain, blocks


@pytest.mark.gpu
def test_single_end_extend_and_mems(exe, medium_case, tmp_path):
    reads = medium_case.synth.make_reads(medium_case.pg, 700, 150, seed=61)
    fq = str(tmp_path / "reads.fastq")
    medium_case.synth.write_fastq(fq, reads)
    prefix = medium_case.path[:-4]
    common = [prefix, "-p", fq, "-S", "1000", "-F", "0.5", "-t", "4", "--gpu-batch", "150", "--ctx-per-gpu", "2"]
    # the streaming front end: five ranges over two contexts, every range's blocks at the prefix sum of the compressed lengths
    plain, blocks = both_ways(exe, common, str(tmp_path / "se.sam"))
    assert plain.count(b"\nsimulated.") + plain.startswith(b"simulated.") >= 700
    assert len(blocks) >= 1 + 5 + 1          # the header's block, at least one per range, the end-of-file block
    # the queue front end (--extend, -m): the writer thread takes the blocks in input order
    both_ways(exe, common + ["--extend"], str(tmp_path / "ext.sam"))
    both_ways(exe, common + ["-m"], str(tmp_path / "mems.sam"))
    # a gzip-compressed read file takes the queue front end too
    fz = str(tmp_path / "reads.fastq.gz")
    with gzip.open(fz, "wb") as f:
        f.write(open(fq, "rb").read())
    plain2, _ = both_ways(exe, [prefix, "-p", fz, "-S", "1000", "-F", "0.5", "-t", "4", "--gpu-batch", "300"], str(tmp_path / "sez.sam"))
    assert plain2 == plain


@pytest.mark.gpu
def test_paired_end(exe, medium_case, tmp_path):
    from tests.test_oracle_pe import make_pairs
    m1, m2, _ = make_pairs(medium_case.pg, 2400, L=100)          # the learning batches' block first, then two batches of the workers
    f1, f2 = str(tmp_path / "m_1.fastq"), str(tmp_path / "m_2.fastq")
    for path, mates, k in ((f1, m1, 1), (f2, m2, 2)):
        with open(path, "wb") as f:
            for i, r in enumerate(mates):
                f.write(b"@p%d/%d\n%s\n+\n%s\n" % (i, k, r.tobytes(), b"I" * len(r)))
    prefix = medium_case.path[:-4]
    args = [prefix, "-1", f1, "-2", f2, "-S", "1000", "-F", "0.5", "-t", "4", "-b", "256", "--gpu-batch", "300", "--ctx-per-gpu", "2"]
    plain, blocks = both_ways(exe, args, str(tmp_path / "pe.sam"))
    assert plain.count(b"\np") >= 4800
    both_ways(exe, args + ["-m"], str(tmp_path / "pe_mems.sam"))
