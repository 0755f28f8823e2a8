"""The strand prefilter's per-lane code (moni_align_amd/csrc/prefilter_core.h) on the host: the k-mer table against a brute-force k-mer set, and the
filter's decisions over packed patterns (pack_task) against an exact bytewise search for a common substring of min_len bytes - no skipped task has
one, at least half of the tasks that have none are skipped where the table is at most 2 % full, nothing is skipped with min_len < k or with a byte
outside A / C / G / T.  A stand-alone program (tests/host_sim/prefilter_sim.cpp), built plain and with the address and undefined-behaviour
sanitizers.  Needs no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_prefilter_sim(tmp_path, flags):
    exe = str(tmp_path / "prefilter_sim")
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "host_sim", "prefilter_sim.cpp")])
    out = subprocess.check_output([exe]).decode()
    assert out.strip().splitlines()[-1].startswith("OK"), out
