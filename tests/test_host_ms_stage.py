"""The two store forms of the seeding walks (moni_align_amd/csrc/seed_core.h) on the host: ms_task over a live list, where a task without its
sister strand stores 16 bytes over both tasks' words, against ms_task over every task; and run_seed (what occ_task runs per seed) with the kept
occurrences staged eight at a time against a store per occurrence.  tests/host_sim/ms_stage_sim.cpp, a program of its own, compares every word of the
workspaces; here its pointers are compared with the oracle's, both strands, no tolerance.  The program is built plain and with the address and
undefined-behaviour sanitizers and run directly.  Needs no GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_sim", "ms_stage_sim.cpp")

# around the pattern word of 8 steps and the 64-step edges, beyond the 160- and 256-base windows of the other seeding kernels, and one read with a depth of its own
LENS = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 150, 151, 200, 300)
COMPL = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCATGCA"):
    COMPL[_a] = _b


def length_mix(mc, n, seed, long_at=None):
    """n reads whose lengths walk through LENS, so that neighbouring tasks end at different steps; every fifth read carries a byte outside
    A / C / G / T at position 0, 7, 8 or at its end (the walk writes sample 0 there); long_at: that read has 2000 bases"""
    base = mc.synth.make_reads(mc.pg, n, 300, seed=seed, sub_rate=0.02)
    reads = []
    for i in range(n):
        r = base[i][:LENS[(i * 7) % len(LENS)]].copy()
        if i % 5 == 4:
            at = (0, 7, 8, len(r) - 1)[(i // 5) % 4]
            if at < len(r):
                r[at] = ord("N")
        reads.append(r)
    if long_at is not None:
        reads[long_at] = np.frombuffer(bytes(mc.fi.text[5000:7000]), dtype=np.uint8).copy()
    return reads


def ragged(reads):
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate(reads).astype(np.uint8), offs


def blob(fi, seq, offs):
    n_seq = len(fi.seq_starts) - 1
    u64 = lambda a: np.ascontiguousarray(a, dtype=np.uint64).tobytes()
    b = u64([fi.n, fi.r, fi.w, n_seq, 1, len(offs) - 1, 0, 0]) + u64(fi.F) + u64(fi.starts) + u64(fi.ssa) + u64(fi.esa) + u64(fi.thr) + u64(fi.slcp)
    return b + u64(fi.seq_starts) + u64(offs) + np.ascontiguousarray(fi.heads, dtype=np.uint8).tobytes() + seq.tobytes()


@pytest.fixture(scope="module")
def batches(medium_case):
    """the batches and the oracle's pointers of their reads, computed once"""
    from oracle import orc
    o = orc.OracleIndex(medium_case.path)
    out = []
    for n, seed, long_at in ((1, 3, None), (33, 4, None), (77, 5, 40)):
        reads = length_mix(medium_case, n, seed, long_at)
        want = np.concatenate([np.concatenate([o.ms_query(r.tobytes()), o.ms_query(COMPL[r[::-1]].tobytes())]) for r in reads])
        out.append((reads, want))
    return out


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_ms_stage_sim(tmp_path, medium_case, batches, flags):
    exe = str(tmp_path / "ms_stage_sim")
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, SRC])
    for reads, want in batches:
        seq, offs = ragged(reads)
        src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
        src.write_bytes(blob(medium_case.fi, seq, offs))
        p = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and p.stdout.strip().splitlines()[-1].startswith("OK") and "runtime error" not in p.stderr, p.stdout + p.stderr[-2000:]
        print(p.stdout.strip())
        nums = [int(x) for x in re.findall(r"\d+", p.stdout.strip().splitlines()[-1])]
        assert 0 < nums[2] < nums[3] and nums[6] > 1000 and nums[7] > 8 * nums[6] // 4 and nums[8] > 100, p.stdout          # listed tasks, walks, kept occurrences, second walks
        raw = np.frombuffer(dst.read_bytes(), dtype=np.uint64)
        assert len(raw) == 2 * int(offs[-1]) + 2
        assert np.array_equal(raw[:-2], want)
        assert int(raw[-2]) == 2 * int(offs[-1])          # a step per base and strand
