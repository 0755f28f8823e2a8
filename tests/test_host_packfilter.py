"""The fused front end of the filtered seeding stage (moni_align_amd/csrc/packfilter_core.h: what pack_filter_kernel runs per read) on the host,
against pack_task + pf_task_keep of the same tree: code, mask and byte words of the workspace, pflag, flag, cnt_m / cnt_s and the lookup count, over
read lengths around every word boundary, batches that fill a 64-task block, leave it partial and spill by one, bytes outside A / C / G / T at the
boundaries, k-mer tables that hold everything, nothing and a fifth, and min_len at, above and below k.  A stand-alone program
(tests/host_sim/packfilter_sim.cpp), built plain and with the address and undefined-behaviour sanitizers.  Needs no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_packfilter_sim(tmp_path, flags):
    exe = str(tmp_path / "packfilter_sim")
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "host_sim", "packfilter_sim.cpp")])
    out = subprocess.check_output([exe]).decode()
    assert out.strip().splitlines()[-1].startswith("OK"), out
