"""The run-level chaining routines of moni_align_amd/csrc/chain_core.h (the DP of one run of anchors, its chain ends and starts, their order, the
backtracking with the keep test, the place of a kept chain among the read's) on the host, through a column accessor of the widths chain_runs_kernel uses: 16-bit f / msc
and 8-bit p / t that hold GLOBAL anchor indices.  tests/host_sim/chain_runs_sim.cpp, a program of its own, draws reads of 1 .. 16 runs of 1 .. AF_RUN_LEN anchors
(tied reference ends, equal runs and so equal scores across runs, both strands, runs with several chain starts and with dropped chains), with max_pred in
{1, 5}, max_iter in {2, 10} and min_chain_score in {0, 20, 40}, and compares f / p / msc of every anchor, the kept chains, their order and their anchor lists
with the whole-read serial form (ac_chain, align_core.h); it chains a run as the first of a read and behind a copy of itself and wants the same chains
(`p > 0` and `t == i` compare global indices), and keeps guard words around every column.  Built plain and with the address and undefined-behaviour
sanitizers and run directly.  Needs no GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_sim", "chain_runs_sim.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_chain_runs_sim(tmp_path, flags):
    exe = str(tmp_path / "chain_runs_sim")
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, SRC])
    seen_starts, seen_kept = {}, {}
    for seed in (1, 2):
        p = subprocess.run([exe, str(seed)], capture_output=True, text=True, timeout=300)
        lines = p.stdout.strip().splitlines()
        assert p.returncode == 0 and lines and lines[-1].startswith("OK") and "runtime error" not in p.stderr, p.stdout + p.stderr[-2000:]
        print(p.stdout.strip())
        for k, v in re.findall(r"(\d+):(\d+)", lines[-4]):
            seen_starts[int(k)] = seen_starts.get(int(k), 0) + int(v)
        for k, v in re.findall(r"(\d+):(\d+)", lines[-3]):
            seen_kept[int(k)] = seen_kept.get(int(k), 0) + int(v)
        dropped, tied, _, many, first = (int(x) for x in re.findall(r"\d+", lines[-2]))
        assert dropped > 1000 and tied > 1000 and first > 1000, lines[-2]
        reads, runs, chains = (int(x) for x in lines[-1].split()[1:])
        assert reads >= 17000 and runs > 5 * reads and chains > reads
    assert all(seen_starts.get(k, 0) > 0 for k in range(8)), seen_starts          # runs without a start, with one, with several
    assert all(seen_kept.get(k, 0) > 0 for k in range(33)), seen_kept            # up to 16 kept chains of a read: one insertion sort; more: the introsort


def test_the_kernel_and_the_simulation_use_the_same_caps():
    fast = open(os.path.join(ROOT, "moni_align_amd", "csrc", "align_fast.hip")).read()
    sim = open(SRC).read()
    caps = re.search(r"RUN_LEN = (\d+), SLOTS = (\d+), MAX_NA = (\d+), MAX_CH = (\d+)", sim).groups()
    assert caps == tuple(re.search(r"#define %s (\d+)" % n, fast).group(1) for n in ("AF_RUN_LEN", "AF_RUN_SLOTS", "AF_RUN_NODES", "AF_RUN_CHAINS"))
