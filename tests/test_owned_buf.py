"""Buf<Tp, Mem> (moni_align_amd/csrc/owned_buf.hpp), the type that owns every device and pinned buffer of the library: ownership, moves, the two
growth rules and ensure_keep, over a counting malloc-backed policy in a stand-alone program built with the address and undefined-behaviour
sanitizers (tests/host_sim/owned_buf_test.cpp).  Needs no GPU: the header does not know the HIP runtime."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owned_buf_under_sanitizers(tmp_path):
    exe = str(tmp_path / "owned_buf_test")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "host_sim", "owned_buf_test.cpp")])
    out = subprocess.check_output([exe]).decode()
    assert out.startswith("OK"), out
