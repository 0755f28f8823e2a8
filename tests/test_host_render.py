"""The per-lane pieces of finish_render_kernel (moni_align_amd/csrc/render_core.h: the segment table and its per-read selects, the digits of a number, the
bytes of one CIGAR operation and of one MD item) compiled for the host: tests/host_sim/render_sim.cpp assembles SAM lines from synthetic recipes lane by
lane, in the kernel's order, and compares every line with a plain snprintf rendering.  The recipes hold what the oracle's inputs never produce (negative
AS and ZS, 10-digit positions) and the edges of the layout: score2 == 0, 0 / 1 / 5 / 16 alternatives, 64 and 128 CIGAR operations, 256 MD items with
deletions, a line of exactly the staging's 1280 bytes and one of 1281.  It is a program of its own, built with the address and undefined-behaviour
sanitizers (their runtimes linked statically: the program needs nothing from its environment).  The kernel itself is checked under -m gpu
(tests/test_gpu_render.py)."""
import os
import re
import subprocess

from moni_align_amd import capi

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sim", "render_sim.cpp")


def test_lines_assembled_lane_by_lane_equal_snprintf_under_sanitizers(tmp_path):
    assert os.path.exists(os.path.join(capi.CSRC, "render_core.h"))
    exe = str(tmp_path / "render_sim_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ERROR" not in p.stderr and "runtime error" not in p.stderr, (p.stdout + p.stderr)[-3000:]
    m = re.search(r"render_sim: (\d+) lines equal, (\d+) of them handed over", p.stdout)
    assert m and int(m.group(1)) > 3000 and int(m.group(2)) >= 3, p.stdout


def test_the_table_and_the_kernel_agree_on_the_literals():
    """the literal table's offsets (LT_*) are positions in one string: each entry of the skeleton that is a literal names the text it is meant to be"""
    text = open(os.path.join(capi.CSRC, "render_core.h")).read()
    lit = re.search(r'#define AFR_LIT_TEXT (.*)', text).group(1)
    s = "".join(bytes(x, "ascii").decode("unicode_escape") for x in re.findall(r'"((?:[^"\\]|\\.)*)"', lit))
    lt = {k: int(v) for k, v in re.findall(r"(LT_[A-Z]+) = (\d+)", text)}
    assert len(s) + 1 == 89
    want = {"LT_TAB": "\t", "LT_MATE": "\t*\t0\t0\t", "LT_AS": "\tAS:i:", "LT_NM": "\tNM:i:", "LT_ZS": "\tZS:i:", "LT_MD": "\tMD:Z:", "LT_OA": "\tOA:Z:", "LT_PLUS": ",+,",
            "LT_MINUS": ",-,", "LT_COMMA": ",", "LT_SEMI": ";", "LT_AA": "\tAA:Z:", "LT_NL": "\n", "LT_UNAL": "\t4\t*\t0\t255\t*\t*\t0\t0\t", "LT_STAR": "*", "LT_CARET": "^",
            "LT_OPS": "MIDNSHP=X", "LT_BASES": "ACGTN"}
    assert set(want) == set(lt)
    for k, v in want.items():
        assert s[lt[k]:lt[k] + len(v)] == v, k
    for at, ln in re.findall(r"AFR_E_LIT\((LT_[A-Z]+), (\d)\)", text):
        assert int(ln) == len(want[at]), at
