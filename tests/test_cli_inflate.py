"""`moni-hip-align` on BGZF input: without a GPU, --dry-run says which input takes the GPU inflater (` input=bgzf`) and the usage text lists
the two options; on the GPU the output of single-end and paired alignment on bgzipped copies of the reads is, byte for byte, the output on the
plain files and the output with --host-inflate, with records and chunks straddling members and calls."""
import gzip
import os
import subprocess

import pytest

from tests import inflate_model as im
from tests.test_host_inflate import TWO_RECORDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "moni_align_amd", "host", "moni-hip-align")


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__
    __graft_entry__.build()
    return EXE


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("blockedin")
    out = {}
    for name, data in (("f.fq", TWO_RECORDS), ("f.fq.bgz", im.bgzip(TWO_RECORDS, eof=True)), ("f.small.bgz", im.bgzip(TWO_RECORDS, 5, eof=True)),
                       ("f.fq.gz", gzip.compress(TWO_RECORDS)), ("wrapped.fa.bgz", im.bgzip(b">a\nACGT\nACGT\n>b\nAC\n")), ("f.fa.bgz", im.bgzip(b">a\nACGTACGT\n>b\nACGT\n"))):
        out[name] = str(d / name)
        open(out[name], "wb").write(data)
    return out


def dry(exe, args):
    return subprocess.check_output([exe, "idx/pref"] + args + ["--dry-run"]).decode()


def test_dry_run_names_the_input(exe, files):
    for name in ("f.fq.bgz", "f.small.bgz"):
        out = dry(exe, ["-p", files[name]])
        assert "reads=2 bases=12" in out and out.rstrip().endswith(" first=a input=bgzf"), out
    assert dry(exe, ["-p", files["f.fa.bgz"]]).rstrip().endswith(" input=bgzf")
    out = dry(exe, ["-p", files["f.fq.bgz"], "--bgzf"])
    assert out.rstrip().endswith(" bgzf=1 input=bgzf")
    out = dry(exe, ["-p", files["f.fq.bgz"], "--bam", "--inflate-blocks", "3"])
    assert out.rstrip().endswith(" bam=1 input=bgzf")
    out = dry(exe, ["-1", files["f.fq.bgz"], "-2", files["f.fq.bgz"], "-o", "pe.sam"])
    assert "pairs=2" in out and out.rstrip().endswith(" second=a input=bgzf")


def test_other_inputs_say_nothing_new(exe, files):
    plain = dry(exe, ["-p", files["f.fq"], "-o", "o.sam"])
    assert "reads=2 bases=12" in plain and "input=" not in plain
    for args in (["-p", files["f.fq.gz"]], ["-p", files["f.fq.bgz"], "--host-inflate"], ["-p", files["wrapped.fa.bgz"]], ["-p", files["f.fq.bgz"], "-m"],
                 ["-p", files["f.fq.bgz"], "-c"], ["-p", files["f.fq.bgz"], "--extend"], ["-p", files["f.fq.bgz"], "--pseudo-ms"], ["-p", files["f.fq.bgz"], "--locate"]):
        out = dry(exe, args + ["-o", "o.sam"])
        assert "input=" not in out and "reads=2" in out, (args, out)
    # the same words as for the plain file
    assert dry(exe, ["-p", files["f.fq.bgz"], "--host-inflate", "-o", "o.sam"]) == plain.replace(files["f.fq"], files["f.fq.bgz"])
    out = dry(exe, ["-1", files["f.fq.bgz"], "-2", files["f.fq.bgz"], "-o", "pe.sam", "--host-inflate"])
    assert "pairs=2" in out and "input=" not in out
    out = dry(exe, ["-1", files["f.fq.gz"], "-2", files["f.fq"], "-o", "pe.sam"])
    assert "pairs=2" in out and "input=" not in out
    out = dry(exe, ["-1", files["f.fq.bgz"], "-2", files["f.fq.bgz"], "-o", "pe.sam", "-m"])
    assert "input=" not in out


def test_usage_lists_them(exe):
    r = subprocess.run([exe, "-h"], capture_output=True)
    assert r.returncode == 1 and b"[--host-inflate]" in r.stderr and b"[--inflate-blocks N]" in r.stderr
    assert b"--host-inflate: BGZF" in r.stderr and b"--inflate-blocks N: BGZF members" in r.stderr


def run(exe, args, out):
    r = subprocess.run([exe] + args + ["-o", out], capture_output=True)
    assert r.returncode == 0, r.stderr
    return r.stderr


@pytest.mark.gpu
def test_single_end(exe, medium_case, tmp_path):
    reads = medium_case.synth.make_reads(medium_case.pg, 700, 150, seed=61)
    fq = str(tmp_path / "reads.fastq")
    medium_case.synth.write_fastq(fq, reads)
    text = open(fq, "rb").read()
    prefix = medium_case.path[:-4]
    common = ["-S", "1000", "-F", "0.5", "-t", "4", "--gpu-batch", "150"]
    run(exe, [prefix, "-p", fq] + common, str(tmp_path / "plain.sam"))
    plain = open(str(tmp_path / "plain.sam"), "rb").read()
    assert plain.startswith(b"@HD") and plain.count(b"\nsimulated.") >= 700
    for k, (bs, extra) in enumerate(((100, ["--inflate-blocks", "3"]), (65280, []), (100, ["--inflate-blocks", "3", "--ctx-per-gpu", "2"]), (4096, ["--inflate-blocks", "7", "--ctx-per-gpu", "1"]))):
        fz = str(tmp_path / ("reads%d.fastq.gz" % k))
        open(fz, "wb").write(im.bgzip(text, bs, eof=True))
        err = run(exe, [prefix, "-p", fz] + common + extra, str(tmp_path / "gpu.sam"))
        assert b"BGZF input" in err, "the run did not take the GPU inflater"
        assert open(str(tmp_path / "gpu.sam"), "rb").read() == plain, (bs, extra)
        err = run(exe, [prefix, "-p", fz, "--host-inflate"] + common + extra, str(tmp_path / "host.sam"))
        assert b"BGZF input" not in err
        assert open(str(tmp_path / "host.sam"), "rb").read() == plain
    # --bgzf on the way out as well
    run(exe, [prefix, "-p", fz, "--bgzf", "--inflate-blocks", "5"] + common, str(tmp_path / "both.sam"))
    assert gzip.decompress(open(str(tmp_path / "both.sam.gz"), "rb").read()) == plain
    # a damaged member stops the run
    z = bytearray(im.bgzip(text, 4096, eof=True))
    z[len(z) // 2] ^= 0x40
    open(fz, "wb").write(bytes(z))
    r = subprocess.run([exe, prefix, "-p", fz, "-o", str(tmp_path / "bad.sam")] + common, capture_output=True)
    assert r.returncode == 1 and b"is damaged" in r.stderr


@pytest.mark.gpu
def test_paired_end(exe, medium_case, tmp_path):
    from tests.test_oracle_pe import make_pairs
    m1, m2, _ = make_pairs(medium_case.pg, 2400, L=100)
    names = {}
    for k, mates in ((1, m1), (2, m2)):
        names[k] = str(tmp_path / ("m_%d.fastq" % k))
        with open(names[k], "wb") as f:
            for i, r in enumerate(mates):
                f.write(b"@p%d/%d\n%s\n+\n%s\n" % (i, k, r.tobytes(), b"I" * len(r)))
    prefix = medium_case.path[:-4]
    common = ["-S", "1000", "-F", "0.5", "-t", "4", "-b", "256", "--gpu-batch", "300", "--ctx-per-gpu", "2"]
    run(exe, [prefix, "-1", names[1], "-2", names[2]] + common, str(tmp_path / "plain.sam"))
    plain = open(str(tmp_path / "plain.sam"), "rb").read()
    assert plain.count(b"\np") >= 4800
    for bs, blocks in ((100, "3"), (65280, "4096")):
        z = {}
        for k in (1, 2):
            z[k] = names[k] + ".%d.gz" % bs
            open(z[k], "wb").write(im.bgzip(open(names[k], "rb").read(), bs + 7 * (k - 1), eof=True))          # the mates' members end at different records
        err = run(exe, [prefix, "-1", z[1], "-2", z[2], "--inflate-blocks", blocks] + common, str(tmp_path / "gpu.sam"))
        assert err.count(b"BGZF input") == 2
        assert open(str(tmp_path / "gpu.sam"), "rb").read() == plain, bs
        run(exe, [prefix, "-1", z[1], "-2", z[2], "--host-inflate"] + common, str(tmp_path / "host.sam"))
        assert open(str(tmp_path / "host.sam"), "rb").read() == plain
    # one mate file blocked, the other plain
    run(exe, [prefix, "-1", z[1], "-2", names[2], "--inflate-blocks", "2"] + common, str(tmp_path / "mixed.sam"))
    assert open(str(tmp_path / "mixed.sam"), "rb").read() == plain
