"""chain_core.h holds the arithmetic of one predecessor of the chaining DP (chain.hpp:300-345) in two forms: the wide one is the reference's 64-bit
arithmetic, the narrow one runs in 32-bit integers on the GPU wherever the host-side predicate cc_narrow_ok admits the parameters.  The stand-alone
program tests/host_sim/chain_core_test.cpp compares the two over l = 0, 1, 2^k - 1, 2^k, 2^k + 1 up to the largest admitted distance, x_d = 0, both mate
cases, average seed lengths of 25 to 512 (non-integers among them) and y_d = 0, +-1, +-(AF_MAX_READ - 1) (and +-(2 * AF_MAX_READ - 1): a pair's second
mate is placed behind the first), at the predicate's own bounds, and checks that the predicate rejects parameters one beyond each bound."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_narrow_form_equals_the_wide_form_where_the_predicate_admits_it(tmp_path):
    exe = str(tmp_path / "chain_core_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host_sim", "chain_core_test.cpp")])
    out = subprocess.check_output([exe]).decode()
    m = re.match(r"OK (\d+)\n", out)
    assert m and int(m.group(1)) > 100000, out


def test_the_bounds_of_the_header_are_the_kernels():
    """the header's own constants against the kernels': reads of the staged path are shorter than AF_MAX_READ"""
    core = open(os.path.join(ROOT, "moni_align_amd", "csrc", "chain_core.h")).read()
    fast = open(os.path.join(ROOT, "moni_align_amd", "csrc", "align_fast.hip")).read()
    assert re.search(r"#define CC_MAX_READ (\d+)", core).group(1) == re.search(r"#define AF_MAX_READ (\d+)", fast).group(1)
