"""`moni-hip-align` on BAM input.  Without a GPU: --dry-run ends with ` input=bam`, the usage text lists --interleaved, and the modes without a BAM
reader refuse it by name.  On the GPU: the output on unaligned BAM made by the model's writer - single end, and pairs from one interleaved file - is,
byte for byte, the output on the FASTQ files, as SAM and as sorted, duplicate-marked BAM; and the tool's own --bam output reads back to the same SAM."""
import os
import subprocess

import pytest

from tests import bamin_model as bm
from tests import inflate_model as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "moni_align_amd", "host", "moni-hip-align")
READS = [(b"a", b"ACGTACGT", 4), (b"s", b"ACGT", 0x104), (b"b", b"ACGT", 0x14)]          # the second is skipped, the third comes back as sequenced


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__
    __graft_entry__.build()
    return EXE


def test_bam_that_is_not_whole_bgzf_is_refused_by_name(exe, tmp_path):
    """zlib reads these, the GPU reader does not: they are refused, not parsed as text and not walked into"""
    import gzip
    raw = bm.header() + b"".join(bm.record(b"p%d" % (i // 2), b"ACGT" * 30, bytes(120), 0x8D if i & 1 else 0x4D) for i in range(400))
    whole = bm.ubam(raw, 4096)
    cases = {"plain_gzip.bam": gzip.compress(raw), "cut.bam": whole[:len(whole) - 40], "tiny.bam": gzip.compress(bm.header(b""))[:27], "trailing.bam": whole + b"xyz"}
    for name, data in cases.items():
        path = str(tmp_path / name)
        open(path, "wb").write(data)
        for args in (["-p", path], ["--interleaved", path], ["-1", path, "-2", path], ["-p", path, "--dry-run"], ["--interleaved", path, "--dry-run"]):
            if name == "tiny.bam" and "--interleaved" not in args:
                continue          # (zlib itself may not give four bytes of so short a file; --interleaved refuses it either way)
            r = subprocess.run([exe, "idx/pref"] + args, capture_output=True)
            assert r.returncode == 1 and (b"BAM input must be whole BGZF members" in r.stderr or b"--interleaved takes a BAM file" in r.stderr), (name, args, r.stderr)
            assert name == "tiny.bam" or b"BAM input must be whole BGZF members" in r.stderr, (name, args, r.stderr)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("bamin")
    single = bm.header() + b"".join(bm.record(n, s, bytes([40]) * len(s), f) for n, s, f in READS)
    pairs = bm.header() + bm.record(b"p", b"ACGTA", bytes(5), 0x4D) + bm.record(b"p", b"GG", bytes(2), 0x8D) + bm.record(b"q", b"TTT", bytes(3), 0x4D) + bm.record(b"q", b"CCCC", bytes(4), 0x8D)
    out = {}
    for name, data in (("s.bam", bm.ubam(single)), ("s.small.bam", bm.ubam(single, 37)), ("p.bam", bm.ubam(pairs)), ("f.fq", b"@a\nACGT\n+\nIIII\n"),
                       ("f.fq.bgz", im.bgzip(b"@a\nACGT\n+\nIIII\n", eof=True))):
        out[name] = str(d / name)
        open(out[name], "wb").write(data)
    return out


def dry(exe, args):
    return subprocess.check_output([exe, "idx/pref"] + args + ["--dry-run"]).decode()


def refused(exe, args, word):
    r = subprocess.run([exe, "idx/pref"] + args, capture_output=True)
    assert r.returncode == 1 and word in r.stderr, (args, r.stderr)


def test_dry_run_names_the_input(exe, files):
    for name in ("s.bam", "s.small.bam"):
        out = dry(exe, ["-p", files[name]])
        assert "reads=2 bases=12" in out and out.rstrip().endswith(" first=a input=bam"), out
    assert dry(exe, ["-p", files["s.bam"], "--bam", "--sort", "--mark-dup"]).rstrip().endswith(" bam=1 sort=1 markdup=1 input=bam")
    out = dry(exe, ["--interleaved", files["p.bam"], "-o", "pe.sam"])
    assert "pairs=2 bases=14" in out and out.rstrip().endswith(" first=p second=p input=bam"), out
    out = dry(exe, ["-1", files["s.bam"], "-2", files["s.bam"], "-o", "pe.sam", "--bgzf"])
    assert "pairs=2 bases=24" in out and out.rstrip().endswith(" first=a second=a bgzf=1 input=bam"), out
    assert "input=" not in dry(exe, ["-p", files["f.fq"], "-o", "o.sam"])
    assert dry(exe, ["-p", files["f.fq.bgz"], "-o", "o.sam"]).rstrip().endswith(" input=bgzf")


def test_usage_lists_interleaved(exe):
    r = subprocess.run([exe, "-h"], capture_output=True)
    assert r.returncode == 1 and b"[--interleaved FILE.bam]" in r.stderr and b"--interleaved FILE.bam: pairs from one BAM" in r.stderr


def test_refusals(exe, files):
    bam, pe = files["s.bam"], files["p.bam"]
    refused(exe, ["-p", bam, "--host-inflate"], b"--host-inflate cannot be combined with BAM input")
    refused(exe, ["--interleaved", pe, "--host-inflate"], b"--host-inflate cannot be combined with BAM input")
    for flag in ("-m", "-c", "--extend", "--ms", "--mems", "--pseudo-ms", "--screen", "--locate", "--seq-count", "--loci"):
        refused(exe, ["-p", bam, flag, "--dry-run"], flag.encode() + b" does not take BAM input")
    refused(exe, ["-p", bam, "--approx", "1"], b"--approx does not take BAM input")
    refused(exe, ["--interleaved", pe, "-m"], b"-m does not take BAM input")
    refused(exe, ["-1", bam, "-2", bam, "-c"], b"-c does not take BAM input")
    for other in (["-p", bam], ["-1", bam], ["-2", bam], ["-1", bam, "-2", bam]):
        refused(exe, ["--interleaved", pe] + other, b"--interleaved cannot be combined with -p, -1 or -2")
    refused(exe, ["--interleaved", files["f.fq"]], b"--interleaved takes a BAM file")
    refused(exe, ["--interleaved", files["f.fq.bgz"]], b"--interleaved takes a BAM file")
    refused(exe, ["-1", bam], b"paired-end alignment needs both -1 and -2")
    refused(exe, ["--interleaved", pe, "--screen"], b"--screen takes single-end input")


def run(exe, args, out):
    r = subprocess.run([exe] + args + ["-o", out], capture_output=True)
    assert r.returncode == 0, r.stderr
    return r.stderr


def fastq_records(text: bytes):
    lines = text.split(b"\n")
    return [(lines[i][1:], lines[i + 1], bytes(c - 33 for c in lines[i + 3])) for i in range(0, len(lines) - 1, 4)]


@pytest.mark.gpu
def test_single_end(exe, medium_case, tmp_path):
    reads = medium_case.synth.make_reads(medium_case.pg, 700, 150, seed=61)
    fq = str(tmp_path / "reads.fastq")
    medium_case.synth.write_fastq(fq, reads)
    recs = fastq_records(open(fq, "rb").read())
    raw = bm.header() + b"".join(bm.record(n, s, q, 4, tags=b"RGZgrp\x00") + (bm.record(n, s[:50], q[:50], 0x104) if i % 7 == 0 else b"") for i, (n, s, q) in enumerate(recs))
    prefix = medium_case.path[:-4]
    common = ["-S", "1000", "-F", "0.5", "-t", "4", "--gpu-batch", "150"]
    run(exe, [prefix, "-p", fq] + common, str(tmp_path / "plain.sam"))
    plain = open(str(tmp_path / "plain.sam"), "rb").read()
    assert plain.startswith(b"@HD") and plain.count(b"\nsimulated.") >= 700
    run(exe, [prefix, "-p", fq, "--bam", "--sort", "--mark-dup"] + common, str(tmp_path / "plain_sorted"))
    for k, (bs, extra) in enumerate(((100, ["--inflate-blocks", "3", "--ctx-per-gpu", "1"]), (65280, ["--inflate-blocks", "3", "--ctx-per-gpu", "2"]))):
        ub = str(tmp_path / ("reads%d.bam" % k))
        open(ub, "wb").write(bm.ubam(raw, bs))
        err = run(exe, [prefix, "-p", ub] + common + extra, str(tmp_path / "gpu.sam"))
        assert b"BAM input" in err, "the run did not take the GPU reader"
        assert open(str(tmp_path / "gpu.sam"), "rb").read() == plain, (bs, extra)
    run(exe, [prefix, "-p", ub, "--bam", "--sort", "--mark-dup"] + common + extra, str(tmp_path / "gpu_sorted"))
    for ext in (".bam", ".bam.bai"):
        assert open(str(tmp_path / "gpu_sorted") + ext, "rb").read() == open(str(tmp_path / "plain_sorted") + ext, "rb").read(), ext
    # the tool's own --bam output (aligned records, reverse strands, CIGARs) read back
    run(exe, [prefix, "-p", fq, "--bam"] + common, str(tmp_path / "own"))
    run(exe, [prefix, "-p", str(tmp_path / "own.bam"), "--inflate-blocks", "2"] + common, str(tmp_path / "again.sam"))
    assert open(str(tmp_path / "again.sam"), "rb").read() == plain
    # a damaged record stops the run with its index and reason
    bad = raw[:len(bm.header())] + b"\x05\x00\x00\x00" + raw[len(bm.header()) + 4:]
    open(ub, "wb").write(bm.ubam(bad, 4096))
    r = subprocess.run([exe, prefix, "-p", ub, "-o", str(tmp_path / "bad.sam")] + common, capture_output=True)
    assert r.returncode == 1 and b"BAM record 0 is refused (reason 3" in r.stderr, r.stderr


@pytest.mark.gpu
def test_interleaved_pairs(exe, medium_case, tmp_path):
    from tests.test_oracle_pe import make_pairs
    m1, m2, _ = make_pairs(medium_case.pg, 2400, L=100)
    names, raw = {}, [bm.header()]
    for k, mates in ((1, m1), (2, m2)):
        names[k] = str(tmp_path / ("m_%d.fastq" % k))
        with open(names[k], "wb") as f:
            for i, r in enumerate(mates):
                f.write(b"@p%d\n%s\n+\n%s\n" % (i, r.tobytes(), b"I" * len(r)))
    for i, (a, b) in enumerate(zip(m1, m2)):
        raw.append(bm.record(b"p%d" % i, a.tobytes(), bytes([40]) * len(a), 0x4D) + bm.record(b"p%d" % i, b.tobytes(), bytes([40]) * len(b), 0x8D))
        if i % 5 == 0:
            raw.append(bm.record(b"p%d" % i, b.tobytes()[:30], bytes(30), 0x8D | 0x800))
    raw = b"".join(raw)
    prefix = medium_case.path[:-4]
    common = ["-S", "1000", "-F", "0.5", "-t", "4", "-b", "256", "--gpu-batch", "300", "--ctx-per-gpu", "2"]
    run(exe, [prefix, "-1", names[1], "-2", names[2]] + common, str(tmp_path / "plain.sam"))
    plain = open(str(tmp_path / "plain.sam"), "rb").read()
    assert plain.count(b"\np") >= 4800
    for bs, blocks in ((100, "3"), (65280, "4096")):
        ub = str(tmp_path / ("pairs%d.bam" % bs))
        open(ub, "wb").write(bm.ubam(raw, bs))
        err = run(exe, [prefix, "--interleaved", ub, "--inflate-blocks", blocks] + common, str(tmp_path / "gpu.sam"))
        assert err.count(b"BAM input") == 1
        assert open(str(tmp_path / "gpu.sam"), "rb").read() == plain, bs
    run(exe, [prefix, "-1", names[1], "-2", names[2], "--bam", "--sort", "--mark-dup"] + common, str(tmp_path / "plain_sorted"))
    run(exe, [prefix, "--interleaved", ub, "--bam", "--sort", "--mark-dup", "--inflate-blocks", "5"] + common, str(tmp_path / "gpu_sorted"))
    for ext in (".bam", ".bam.bai"):
        assert open(str(tmp_path / "gpu_sorted") + ext, "rb").read() == open(str(tmp_path / "plain_sorted") + ext, "rb").read(), ext
    # a file sorted by coordinate is no input for pairs
    srt = bm.header() + bm.record(b"a", b"ACGT", bytes(4), 0x41) + bm.record(b"b", b"ACGT", bytes(4), 0x41) + bm.record(b"a", b"ACGT", bytes(4), 0x81) + bm.record(b"b", b"ACGT", bytes(4), 0x81)
    open(ub, "wb").write(bm.ubam(srt))
    r = subprocess.run([exe, prefix, "--interleaved", ub, "-o", str(tmp_path / "bad.sam")] + common, capture_output=True)
    assert r.returncode == 1 and b"BAM record 1 is refused (reason 5" in r.stderr and b"samtools collate" in r.stderr, r.stderr
