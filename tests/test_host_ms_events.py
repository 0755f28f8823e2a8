"""The event lists of the seeding walk (moni_align_amd/csrc/seed_core.h) on the host: ms_task_events records the assignments of a walk - threshold jumps
and absent bytes - where ms_task stores a pointer per step, and mem_task rebuilds the pointers from them.  tests/host_sim/ms_events_sim.cpp, a program
of its own, expands every list and compares it word for word with ms_task's pointers, checks guard words around the lists, the counts and the stage,
and runs mem_task from the dense and the event source (with and without the closed form over silent offsets), count pass and emit pass; here its
pointers are compared with the oracle's, both strands, no tolerance, and the lists must have the lengths at which the stage of eight flushes.  The
program is built plain and with the address and undefined-behaviour sanitizers and run directly.  Needs no GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_host_ms_stage import COMPL, LENS, length_mix, ragged

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_sim", "ms_events_sim.cpp")
EDGES = (1, 7, 8, 9, 16, 17)          # events of a list: one, around one line of the stage, around two


def event_counts(pointers, lens):
    """events per task from the dense pointers in moni_ms_query_batch's order (per read strand 0, then strand 1, each by read offset): one for the start
    and one wherever a pointer is not its right neighbour's minus one.  A lower bound that misses only a jump onto exactly that value."""
    out, at = [], 0
    for m in lens:
        for _ in range(2):
            p = pointers[at:at + m]
            out.append(1 + int(np.count_nonzero(p[:-1] + np.uint64(1) != p[1:])) if m else 0)
            at += m
    return out


def edge_mix(mc, seed):
    """reads whose lists have every length of EDGES: copies of the text (a list of one or a few events on the strand that occurs, a jump at nearly
    every step on the other), random reads of 7 to 40 bases, the mixed lengths of the stage's tests with their bytes outside A / C / G / T, and a byte
    >= 0x80 and an N each followed by bases that match (the decrement of 0 wraps)"""
    rng = np.random.default_rng(seed)
    text = np.frombuffer(bytes(mc.fi.text), dtype=np.uint8)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    reads = []
    for i in range(40):
        m = (1, 7, 8, 9, 16, 17, 40, 150)[i % 8]
        at = int(rng.integers(1000, len(text) - 1000))
        r = text[at:at + m].copy()
        if not np.isin(r, acgt).all():
            r = acgt[rng.integers(0, 4, size=m)]
        reads.append(r)
    for i in range(60):
        reads.append(acgt[rng.integers(0, 4, size=7 + (i * 5) % 34)])
    reads += length_mix(mc, 45, seed)
    for byte in (0x80, ord("N"), 0xFF):
        at = int(rng.integers(1000, len(text) - 1000))
        r = text[at:at + 150].copy()
        r[149] = byte; r[40] = byte; r[0] = byte          # the first step of strand 0, the last of strand 1; 40 and 0: matching bases follow on strand 0
        reads.append(r)
    order = rng.permutation(len(reads))                   # neighbouring lanes differ
    return [reads[k] for k in order]


def blob(fi, seq, offs):
    n_seq = len(fi.seq_starts) - 1
    u64 = lambda a: np.ascontiguousarray(a, dtype=np.uint64).tobytes()
    b = u64([fi.n, fi.r, fi.w, n_seq, 1, len(offs) - 1, 0, 0]) + u64(fi.F) + u64(fi.starts) + u64(fi.ssa) + u64(fi.esa) + u64(fi.thr) + u64(fi.slcp)
    return b + u64(fi.seq_starts) + u64(offs) + np.ascontiguousarray(fi.heads, dtype=np.uint8).tobytes() + seq.tobytes() + bytes(fi.text)[:fi.n - 1]


@pytest.fixture(scope="module")
def batches(medium_case):
    """the batches and the oracle's pointers of their reads, computed once"""
    from oracle import orc
    o = orc.OracleIndex(medium_case.path)
    out = []
    for reads in (length_mix(medium_case, 1, 3), length_mix(medium_case, 33, 4), edge_mix(medium_case, 5)):
        want = np.concatenate([np.concatenate([o.ms_query(r.tobytes()), o.ms_query(COMPL[r[::-1]].tobytes())]) for r in reads])
        out.append((reads, want))
    return out


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_ms_events_sim(tmp_path, medium_case, batches, flags):
    exe = str(tmp_path / "ms_events_sim")
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, SRC])
    seen = {}
    for reads, want in batches:
        seq, offs = ragged(reads)
        src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
        src.write_bytes(blob(medium_case.fi, seq, offs))
        p = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
        lines = p.stdout.strip().splitlines()
        assert p.returncode == 0 and lines[-1].startswith("OK") and "runtime error" not in p.stderr, p.stdout + p.stderr[-2000:]
        print(p.stdout.strip())
        raw = np.frombuffer(dst.read_bytes(), dtype=np.uint64)
        assert len(raw) == 2 * int(offs[-1]) + 2
        assert np.array_equal(raw[:-2], want)
        assert int(raw[-2]) == 2 * int(offs[-1])          # a step per base and strand
        hist = {int(a): int(b) for a, b in re.findall(r"(\d+):(\d+)", lines[-2])}
        for k, v in hist.items():
            seen[k] = seen.get(k, 0) + v
        nums = [int(x) for x in re.findall(r"\d+", lines[-1])]
        assert nums[3] == sum(k * v for k, v in hist.items()) >= sum(event_counts(want, [len(r) for r in reads]))
    for k in EDGES:
        assert seen.get(k, 0) > 0, (k, sorted(seen))
    assert max(seen) > 32 and nums[4] > 0 and nums[9] > 0, lines          # a long list, wrapped words, tasks the emit pass walks again
