"""The leaping walk of the seeding stage (moni_align_amd/csrc/seed_core.h: ms_task_events_leap, isa_walk_run, leap_clean_chunk) on the host.
tests/host_sim/ms_leap_sim.cpp, a program of its own, makes a suffix array of the text, proves that the walk's BWT position is ISA[sample] at every
step the leap relies on, compares every entry of the sampled inverse suffix array (strides 8, 16, 32) with it, and runs the leaping walk against
the stepwise one: event lists word for word, counts, steps and jumps, all tasks and over a live list.  Here the batch is put together - the batches
of test_host_ms_events.py and the edge reads of the leap - and what the program reports is checked: the stretch lengths around the thresholds occur,
leapable stretches end on a multiple of the stride, and every exact 150-base copy of the text leaps.  The program is built plain and with the
address and undefined-behaviour sanitizers and run directly.  Needs no GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_host_ms_events import blob, edge_mix
from tests.test_host_ms_stage import length_mix, ragged

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_sim", "ms_leap_sim.cpp")
T, K_MIN, STRIDES, DEFAULT_STRIDE = 8, 8, (8, 16, 32), 16          # seed_core.h: MONI_LEAP_T, MONI_LEAP_KMIN, MONI_LEAP_SH
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def clean_at(text, rng, m):
    """a place where m bytes of the text are all A / C / G / T"""
    while True:
        at = int(rng.integers(0, len(text) - m))
        if np.isin(text[at:at + m], ACGT).all():
            return at


def other(b, rng):
    return ACGT[(int(np.where(ACGT == b)[0][0]) + int(rng.integers(1, 4))) % 4]


def leap_mix(case, seed, n_copies):
    """the edge reads of the leap; returns the reads and the indices of those that are exact 150-base copies of the text (A / C / G / T only)"""
    rng = np.random.default_rng(seed)
    text = np.frombuffer(bytes(case.fi.text), dtype=np.uint8)[:case.fi.n - 1]
    ss = [int(x) for x in case.fi.seq_starts]
    reads, exact = [], []
    for _ in range(n_copies):                                 # exact copies
        at = clean_at(text, rng, 150)
        exact.append(len(reads)); reads.append(text[at:at + 150].copy())
    for at in [0] + ss[1:-1]:                                 # copies that start at text position 0 and at a sequence start
        r = text[at:at + 150].copy()
        if np.isin(r, ACGT).all():
            exact.append(len(reads))
        reads.append(r)
    for at in ss[1:-1]:                                       # a copy across a separator
        reads.append(text[at - 75:at + 75].copy())
    for d in range(1, 72):                                    # two substitutions d apart: the matched stretch between them has every length around T and T + stride + K_MIN
        for rep in range(2):
            at = clean_at(text, rng, 150)
            r = text[at:at + 150].copy()
            hi = 140 - int(rng.integers(0, 8)) * rep
            for p in (hi, hi - d):
                r[p] = other(r[p], rng)
            reads.append(r)
    for m in range(1, T + 2):                                 # read lengths 1 .. T + 1
        at = clean_at(text, rng, m)
        reads.append(text[at:at + m].copy())
    for k in range(6):                                        # 250 bases: copies, and copies with one substitution
        at = clean_at(text, rng, 250)
        r = text[at:at + 250].copy()
        if k % 2:
            r[int(rng.integers(20, 230))] = ord("A") if r[100] != ord("A") else ord("C")
        reads.append(r)
    for byte in (ord("N"), 0x80, 0xFF):                       # a byte outside A / C / G / T inside a long stretch
        at = clean_at(text, rng, 150)
        r = text[at:at + 150].copy()
        r[int(rng.integers(60, 90))] = byte
        reads.append(r)
    order = rng.permutation(len(reads))                       # neighbouring lanes differ
    where = {int(k): i for i, k in enumerate(order)}
    return [reads[k] for k in order], sorted(where[i] for i in exact)


@pytest.fixture(scope="module", params=[["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ms_leap") / "ms_leap_sim")
    subprocess.check_call(["g++", "-std=c++17"] + request.param + ["-o", out, SRC])
    return out


def run_sim(exe, tmp_path, case, reads):
    seq, offs = ragged(reads)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(blob(case.fi, seq, offs))
    p = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=600)
    lines = p.stdout.strip().splitlines()
    assert p.returncode == 0 and lines and lines[-1].startswith("OK") and "runtime error" not in p.stderr, p.stdout + p.stderr[-2000:]
    print(p.stdout.strip())
    leaps = np.frombuffer(dst.read_bytes(), dtype=np.uint32)
    assert len(leaps) == 2 * len(reads)
    stretches = {int(x) for x in lines[-4].split(":")[1].split()}
    on_mult = {int(s): (int(a), int(b)) for s, a, b in re.findall(r"(\d+): (\d+) \((\d+)\)", lines[-3])}
    stats = {int(s): (int(a), int(b), int(c)) for s, a, b, c in re.findall(r"(\d+): (\d+) (\d+) (\d+)", lines[-2])}
    return leaps, stretches, on_mult, stats, [int(x) for x in re.findall(r"\d+", lines[-1])]


def test_ms_leap_sim_small(exe, tmp_path, small_case):
    """the tables of the small index, and a small batch of the edge reads"""
    reads, exact = leap_mix(small_case, 11, 10)
    leaps, _, _, stats, nums = run_sim(exe, tmp_path, small_case, reads)
    assert nums[3] > 0 and all(stats[s][0] > 0 for s in STRIDES), (nums, stats)
    for i in exact:
        assert leaps[2 * i] >= 1, (i, bytes(reads[i]))


def test_ms_leap_sim_medium(exe, tmp_path, medium_case):
    edge, exact = leap_mix(medium_case, 6, 40)
    head = length_mix(medium_case, 33, 4) + edge_mix(medium_case, 5)
    reads = head + edge
    leaps, stretches, on_mult, stats, nums = run_sim(exe, tmp_path, medium_case, reads)
    for s in STRIDES:                                         # the stretch lengths on both sides of the two thresholds, at every stride
        for want in (T - 1, T, T + s + K_MIN - 1, T + s + K_MIN):
            assert want in stretches, (want, sorted(stretches))
        assert on_mult[s][1] > 0, on_mult                     # a leapable stretch that ends exactly on a multiple of the stride
        assert stats[s][0] > 0 and stats[s][1] >= stats[s][0] * (K_MIN + 1) and stats[s][2] >= stats[s][0], stats
    assert nums[4] > 0                                        # steps behind an absent byte, where the relation does not hold
    for i in exact:                                           # not vacuous: every exact 150-base copy leaps on its forward strand
        assert leaps[2 * (len(head) + i)] >= 1, (i, bytes(edge[i]))
