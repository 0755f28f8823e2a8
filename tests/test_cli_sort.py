"""`moni-hip-align --bam --sort`: without a GPU the option parses (--dry-run says sort=1), is listed by the usage text, belongs to --bam and
refuses what --bam refuses, and changes nothing where it is not given; on the GPU <out>.bam holds, under an SO:coordinate header, the model's
sort (tests/bamsort_model.sort) of the plain --bam run's records, the same bytes for every batch size and number of contexts; <out>.bam.bai
is the model's index of the very file written, and the strict reader finds through it what a scan of the file finds."""
import gzip
import os
import subprocess

import pytest

from tests import bam_model as bam
from tests import bamsort_model as bsm
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
    p = str(tmp_path_factory.mktemp("records") / "f.fq")
    open(p, "w").write("@a\nACGTACGT\n+\nIIIIIIII\n@b\nACGT\n+\nIIII\n")
    return p


def test_dry_run_says_sort(exe, fq):
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "-o", "o.sam", "--bam", "--sort", "--dry-run"]).decode()
    assert out.rstrip().endswith(" bam=1 sort=1") and "Output file: o.bam\n" in out
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "-o", "o.sam", "--bam", "--sort", "--sort-chunk", "65536", "--extend", "--dry-run"]).decode()
    assert " bam=1 sort=1" in out and "mode=extend" in out
    out = subprocess.check_output([exe, "idx/pref", "-1", fq, "-2", fq, "-o", "pe.sam", "--sort", "--bam", "--dry-run"]).decode()
    assert "pairs=2" in out and out.rstrip().endswith("bam=1 sort=1") and "Output file: pe.bam\n" in out


def test_without_the_option_nothing_changes(exe, fq):
    for args in (["-p", fq, "--bam"], ["-p", fq], ["-1", fq, "-2", fq, "-o", "pe.sam", "--bam"], ["-p", fq, "-o", "o", "--extend", "--bam"], ["-p", fq, "--bgzf"]):
        out = subprocess.check_output([exe, "idx/pref"] + args + ["--dry-run"]).decode()
        assert "sort" not in out
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "--bam", "--dry-run"]).decode()
    assert out.rstrip().endswith(" bam=1") and ("out=%s_pref_25.bam first=a bam=1\n" % fq) in out
    out = subprocess.check_output([exe, "idx/pref", "-1", fq, "-2", fq, "-o", "pe.sam", "--bam", "--dry-run"]).decode()
    assert out.rstrip().endswith("out=pe.bam first=a second=a bam=1")


@pytest.mark.parametrize("extra,word", [([], b"--sort belongs to --bam"), (["--bam", "--bgzf"], b"--sort cannot be combined with --bgzf"),
                                        (["--bam", "-c"], b"--sort cannot be combined with -c"), (["--bam", "--dry-run-write"], b"--sort cannot be combined with --dry-run-write"),
                                        (["--bam", "--ms"], b"--sort cannot be combined with --ms"), (["--bam", "--mems"], b"--sort cannot be combined with --mems"),
                                        (["--bam", "--pseudo-ms"], b"--sort cannot be combined with --pseudo-ms"), (["--bam", "--screen"], b"--sort cannot be combined with --screen"),
                                        (["--bam", "--locate"], b"--sort cannot be combined with --locate"), (["--bam", "--seq-count"], b"--sort cannot be combined with --seq-count"),
                                        (["--bam", "--loci"], b"--sort cannot be combined with --loci"), (["--bam", "--approx", "1"], b"--sort cannot be combined with --approx"),
                                        (["--bam", "--sort-chunk", "65535"], b"--sort-chunk takes at least 65536")])
def test_refuses(exe, fq, tmp_path, extra, word):
    out = str(tmp_path / "o.sam")
    r = subprocess.run([exe, "x", "-p", fq, "-o", out, "--sort"] + extra, capture_output=True)
    assert r.returncode == 1 and word in r.stderr, (extra, r.stderr)
    assert not os.listdir(str(tmp_path))


def test_sort_chunk_belongs_to_sort(exe, fq, tmp_path):
    r = subprocess.run([exe, "x", "-p", fq, "-o", str(tmp_path / "o.sam"), "--bam", "--sort-chunk", "65536"], capture_output=True)
    assert r.returncode == 1 and b"--sort-chunk belongs to --sort" in r.stderr and not os.listdir(str(tmp_path))


def test_usage_lists_it(exe):
    r = subprocess.run([exe, "-h"], capture_output=True)
    assert r.returncode == 1 and b"[--sort [--sort-chunk BYTES]]" in r.stderr and b"--sort: with --bam" in r.stderr and b"--sort-chunk BYTES:" in r.stderr


def run(exe, args, out, extra):
    r = subprocess.run([exe] + args + ["-o", out] + extra, capture_output=True)
    assert r.returncode == 0, r.stderr
    return open(out[:-4] + ".bam", "rb").read()


def sorted_ways(exe, args, tmp_path, name, configs, regions=12):
    """the plain --bam run, then --bam --sort in every configuration: one file, the model's; its index, the model's; queries through it"""
    d = str(tmp_path / name)
    os.mkdir(d)
    unsorted = gzip.decompress(run(exe, args + configs[0], os.path.join(d, "plain.sam"), ["--bam"]))
    text = bam.decode(unsorted)          # the strict reader takes it
    header, _ = bam.split_sam(text)
    assert b"SO:unknown" in header.split(b"\n")[0]
    records = unsorted[len(bam.encode_header(header)):]
    n_ref = len(bam.references(header))
    want_header = bsm.coordinate_header(header)
    want = bam.encode_header(want_header) + bsm.sort(header, records)
    assert bsm.sort(header, records) != records and len(bsm.split_records(records)) > 1000
    first = None
    for k, cfg in enumerate(configs):
        out = os.path.join(d, "s%d.sam" % k)
        z = run(exe, args + cfg, out, ["--bam", "--sort", "--sort-chunk", "65536"])
        assert z.endswith(bm.EOF_BLOCK) and sorted(os.listdir(d)) == sorted(["plain.bam"] + [f for j in range(k + 1) for f in ("s%d.bam" % j, "s%d.bam.bai" % j)]), os.listdir(d)
        blocks = bm.walk(z)
        assert b"".join(b for b, _ in blocks) == want, "configuration %r" % (cfg,)
        assert blocks[0][0] == bam.encode_header(want_header) and b"SO:coordinate" in bam.decode(want).split(b"\n")[0]
        bai = open(out[:-4] + ".bam.bai", "rb").read()
        assert bai == bsm.bai_build(z), "the index is not the model's of the file written (configuration %r)" % (cfg,)
        if first is None:
            first = (z, bai)
            assert len(blocks) > 12          # the header, more than ten chunks of 64 KiB, the end-of-file block
    z, bai = first
    f = bsm.BamFile(z)
    placed = [bsm.fields(r) for r in f.recs if bsm.fields(r)[0] >= 0]
    assert placed and n_ref >= 1
    step = max(1, len(placed) // regions)
    asked = 0
    for ref, pos, end, _, _ in placed[::step][:regions]:
        for beg, stop in ((pos, pos + 1), (max(pos - 300, 0), end + 300), (pos >> 14 << 14, (pos >> 14 << 14) + 16384)):
            got = bsm.bai_query(bai, z, ref, beg, stop)
            assert got == bsm.brute_query(z, ref, beg, stop) and (got or beg != pos)
            asked += 1
    assert asked >= 12
    assert bsm.bai_query(bai, z, 0, (1 << 29) - 10, 1 << 29) == []
    return want


@pytest.fixture(scope="module")
def reads_fq(medium_case, tmp_path_factory):
    """6000 reads, and the first 3000 of them"""
    d = tmp_path_factory.mktemp("sorted")
    reads = medium_case.synth.make_reads(medium_case.pg, 6000, 150, seed=61)
    medium_case.synth.write_fastq(str(d / "reads.fastq"), reads)
    medium_case.synth.write_fastq(str(d / "half.fastq"), reads[:3000])
    return str(d / "reads.fastq"), str(d / "half.fastq")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ([], ["--extend"], ["-m"]), ids=("align", "extend", "mems"))
def test_single_end(exe, medium_case, reads_fq, tmp_path, mode):
    """twelve runs and more than ten chunks; another batch size; one context against three.  Plain alignment takes the streaming front end
    (6000 reads, ranges of 500), the other two modes the queue front end (3000 reads, batches of 250: -m writes several records per read)"""
    fq, batch = (reads_fq[0], 500) if not mode else (reads_fq[1], 250)
    common = [medium_case.path[:-4], "-p", fq, "-S", "1000", "-F", "0.5", "-t", "4"] + mode
    configs = [["--gpu-batch", str(batch), "--ctx-per-gpu", "3"], ["--gpu-batch", str(batch), "--ctx-per-gpu", "1"], ["--gpu-batch", str(13 * batch // 5), "--ctx-per-gpu", "3"]]
    sorted_ways(exe, common, tmp_path, "se", configs if not mode else configs[::2])


@pytest.mark.gpu
def test_paired_end(exe, medium_case, tmp_path):
    from tests.test_oracle_pe import make_pairs
    m1, m2, _ = make_pairs(medium_case.pg, 3000, L=100)
    f1, f2 = str(tmp_path / "m_1.fastq"), str(tmp_path / "m_2.fastq")
    for path, mates, k in ((f1, m1, 1), (f2, m2, 2)):
        with open(path, "wb") as f:
            for i, r in enumerate(mates):
                f.write(b"@p%d/%d\n%s\n+\n%s\n" % (i, k, r.tobytes(), b"I" * len(r)))
    prefix = medium_case.path[:-4]
    args = [prefix, "-1", f1, "-2", f2, "-S", "1000", "-F", "0.5", "-t", "4", "-b", "256"]
    sorted_ways(exe, args, tmp_path, "pe", [["--gpu-batch", "500", "--ctx-per-gpu", "3"], ["--gpu-batch", "500", "--ctx-per-gpu", "1"], ["--gpu-batch", "2600", "--ctx-per-gpu", "2"]])
