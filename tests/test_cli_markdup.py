"""`moni-hip-align --bam --sort --mark-dup`: without a GPU the option parses (--dry-run says markdup=1 behind sort=1), is listed by the usage text,
belongs to --sort, refuses the modes that write several records per read, and changes nothing where it is not given; on the GPU <out>.bam holds
the model's sort (tests/bamsort_model.sort) of the plain --bam run's records after tests/markdup_model has set their flags - the same bytes for
every batch size and number of contexts -, <out>.bam.bai is the model's index of the very file written, and the summary line carries the
model's numbers.  A tenth of the reads is planted a second time under another name with other qualities, 7 to 2000 reads later, so that
copies fall into other batches."""
import gzip
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import bam_model as bam
from tests import bamsort_model as bsm
from tests import bgzf_model as bm
from tests import markdup_model as md

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


def test_dry_run_says_markdup(exe, fq):
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "-o", "o.sam", "--bam", "--sort", "--mark-dup", "--dry-run"]).decode()
    assert out.rstrip().endswith(" bam=1 sort=1 markdup=1") and "Output file: o.bam\n" in out
    out = subprocess.check_output([exe, "idx/pref", "-1", fq, "-2", fq, "-o", "pe.sam", "--mark-dup", "--sort", "--bam", "--dry-run"]).decode()
    assert "pairs=2" in out and out.rstrip().endswith("bam=1 sort=1 markdup=1") and "Output file: pe.bam\n" in out


def test_without_the_option_nothing_changes(exe, fq):
    for args in (["-p", fq, "--bam", "--sort"], ["-p", fq, "--bam"], ["-p", fq], ["-1", fq, "-2", fq, "-o", "pe.sam", "--bam", "--sort"], ["-p", fq, "-o", "o", "--extend", "--bam", "--sort"],
                 ["-p", fq, "--bgzf"]):
        out = subprocess.check_output([exe, "idx/pref"] + args + ["--dry-run"]).decode()
        assert "markdup" not in out
    out = subprocess.check_output([exe, "idx/pref", "-p", fq, "--bam", "--sort", "--dry-run"]).decode()
    assert out.rstrip().endswith(" bam=1 sort=1") and ("out=%s_pref_25.bam first=a bam=1 sort=1\n" % fq) in out
    out = subprocess.check_output([exe, "idx/pref", "-1", fq, "-2", fq, "-o", "pe.sam", "--bam", "--sort", "--dry-run"]).decode()
    assert out.rstrip().endswith("out=pe.bam first=a second=a bam=1 sort=1")


@pytest.mark.parametrize("extra,word", [(["--bam"], b"--mark-dup belongs to --sort"), ([], b"--mark-dup belongs to --sort"),
                                        (["--bam", "--sort", "--extend"], b"--mark-dup cannot be combined with --extend"),
                                        (["--bam", "--sort", "-m"], b"--mark-dup cannot be combined with -m"),
                                        (["--sort"], b"--sort belongs to --bam")])
def test_refuses(exe, fq, tmp_path, extra, word):
    out = str(tmp_path / "o.sam")
    r = subprocess.run([exe, "x", "-p", fq, "-o", out, "--mark-dup"] + extra, capture_output=True)
    assert r.returncode == 1 and word in r.stderr, (extra, r.stderr)
    assert not os.listdir(str(tmp_path))


def test_usage_lists_it(exe):
    r = subprocess.run([exe, "-h"], capture_output=True)
    assert r.returncode == 1 and b"[--sort [--sort-chunk BYTES]] [--mark-dup]" in r.stderr and b"--mark-dup: with --sort" in r.stderr


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------------------

def planted(n, share, seed):
    """the order of an input of n units of which every share-th comes twice: [(unit, is the copy)], the copy 7 to 2000 places behind its original"""
    rng = np.random.default_rng(seed)
    keyed = [(float(i), i, False) for i in range(n)]
    keyed += [(i + int(rng.integers(7, 2001)) + 0.5, i, True) for i in range(0, n, share)]
    keyed.sort(key=lambda x: x[0])          # stable: a copy lands behind the original at that place
    return [(i, copy) for _, i, copy in keyed]


def quals(rng, n):
    """varied qualities: Phred 2 to 40, so that some lie below 15"""
    return bytes((33 + rng.integers(2, 41, size=n)).astype(np.uint8))


def run(exe, args, out, extra):
    r = subprocess.run([exe] + args + ["-o", out] + extra, capture_output=True)
    assert r.returncode == 0, r.stderr
    return open(out[:-4] + ".bam", "rb").read(), r.stdout


def flags_of(rec):
    return struct.unpack_from("<H", rec, 18)[0]


def marked_ways(exe, args, tmp_path, name, configs, paired, order, batch_units):
    """the plain --bam run, then --bam --sort --mark-dup in every configuration: one file, the model's; its index, the model's; the summary line"""
    d = str(tmp_path / name)
    os.mkdir(d)
    unsorted = gzip.decompress(run(exe, args + configs[0], os.path.join(d, "plain.sam"), ["--bam"])[0])
    header, _ = bam.split_sam(bam.decode(unsorted))
    n_ref = len(bam.references(header))
    recs = bsm.split_records(unsorted[len(bam.encode_header(header)):])
    per = 2 if paired else 1
    assert len(recs) == per * len(order)
    # the planted copies whose original and copy are both mapped and primary: at least so many records must be marked
    at = {}
    for k, (i, copy) in enumerate(order):
        at.setdefault(i, []).append(k)
    ok = lambda k: all(not flags_of(recs[per * k + x]) & 0x904 for x in range(per))
    both = sum(1 for i, ks in at.items() if len(ks) == 2 and ok(ks[0]) and ok(ks[1]))
    assert both >= 100, "%d planted copies with both the original and the copy mapped" % both
    assert any(abs(ks[1] - ks[0]) > batch_units for ks in at.values() if len(ks) == 2), "no copy fell into another batch"
    ents = md.entries(recs, paired, n_ref)          # the whole input as one run: the output does not depend on the batches
    marked = md.resolve([ents])
    assert len(marked) >= both * per
    p, dp, f, df, m = md.counts([ents], marked)
    want_records = bsm.sort_list(n_ref, md.set_flags(recs, [i for _, i in marked]))
    want = bam.encode_header(bsm.coordinate_header(header)) + b"".join(want_records)
    summary = ("Duplicates: %d of %d pairs, %d of %d fragments, %d records marked" % (dp, p, df, f, m)).encode()
    for k, cfg in enumerate(configs):
        out = os.path.join(d, "s%d.sam" % k)
        z, stdout = run(exe, args + cfg, out, ["--bam", "--sort", "--sort-chunk", "65536", "--mark-dup"])
        assert z.endswith(bm.EOF_BLOCK) and sorted(os.listdir(d)) == sorted(["plain.bam"] + [f_ for j in range(k + 1) for f_ in ("s%d.bam" % j, "s%d.bam.bai" % j)]), os.listdir(d)
        got = b"".join(b for b, _ in bm.walk(z))
        assert got == want, "configuration %r" % (cfg,)
        assert open(out[:-4] + ".bam.bai", "rb").read() == bsm.bai_build(z), "the index is not the model's of the file written (configuration %r)" % (cfg,)
        assert summary in stdout, (summary, re.findall(rb"Duplicates:[^\n]*", stdout))
    # without the option the sorted file carries no 0x400 and is the model's plain sort
    z, stdout = run(exe, args + configs[0], os.path.join(d, "n.sam"), ["--bam", "--sort", "--sort-chunk", "65536"])
    assert b"".join(b for b, _ in bm.walk(z)) == bam.encode_header(bsm.coordinate_header(header)) + bsm.sort(header, b"".join(recs)) and b"Duplicates:" not in stdout
    return m


@pytest.mark.gpu
def test_single_end(exe, medium_case, tmp_path):
    """3000 reads and 300 copies in batches of 250; another batch size; one context against three"""
    reads = medium_case.synth.make_reads(medium_case.pg, 3000, 150, seed=61)
    order = planted(3000, 10, 7)
    rng = np.random.default_rng(11)
    fq = str(tmp_path / "reads.fastq")
    with open(fq, "wb") as f:
        for i, copy in order:
            f.write(b"@%s.%d\n%s\n+\n%s\n" % (b"copy" if copy else b"read", i, reads[i].tobytes(), quals(rng, 150)))
    common = [medium_case.path[:-4], "-p", fq, "-S", "1000", "-F", "0.5", "-t", "4"]
    configs = [["--gpu-batch", "250", "--ctx-per-gpu", "3"], ["--gpu-batch", "250", "--ctx-per-gpu", "1"], ["--gpu-batch", "650", "--ctx-per-gpu", "3"]]
    assert marked_ways(exe, common, tmp_path, "se", configs, False, order, 250) >= 100


@pytest.mark.gpu
def test_paired_end(exe, medium_case, tmp_path):
    """3000 pairs and 300 copies"""
    from tests.test_oracle_pe import make_pairs
    m1, m2, _ = make_pairs(medium_case.pg, 3000, L=100)
    order = planted(3000, 10, 9)
    rng = np.random.default_rng(13)
    f1, f2 = str(tmp_path / "m_1.fastq"), str(tmp_path / "m_2.fastq")
    with open(f1, "wb") as a, open(f2, "wb") as b:
        for i, copy in order:
            for f, mates, k in ((a, m1, 1), (b, m2, 2)):
                f.write(b"@%s%d/%d\n%s\n+\n%s\n" % (b"c" if copy else b"p", i, k, mates[i].tobytes(), quals(rng, len(mates[i]))))
    args = [medium_case.path[:-4], "-1", f1, "-2", f2, "-S", "1000", "-F", "0.5", "-t", "4", "-b", "256"]
    configs = [["--gpu-batch", "500", "--ctx-per-gpu", "3"], ["--gpu-batch", "500", "--ctx-per-gpu", "1"], ["--gpu-batch", "2600", "--ctx-per-gpu", "2"]]
    assert marked_ways(exe, args, tmp_path, "pe", configs, True, order, 1024) >= 200
