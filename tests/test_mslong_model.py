"""The surface that matching statistics of long patterns adds, checked without a GPU: the exported symbols and their ctypes mirrors, the argument
checks that need no device, the defaults, and `moni-hip-align --split`, which belongs to --ms / --mems.  (The per-lane code is replayed against the
oracle in tests/test_host_mslong.py, the kernels run in tests/test_gpu_mslong.py.)"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from moni_align_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "moni_align_amd", "host", "moni-hip-align")


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__
    __graft_entry__.build()
    return EXE


@pytest.fixture(scope="module")
def fa(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("mslong") / "p.fa")
    open(p, "w").write(">a\nACGTACGTACGTACGT\n>b\nACGT\n")
    return p


def test_abi_surface():
    hdr = open(os.path.join(ROOT, "include", "moni_hip.h")).read()
    assert re.search(r"\bvoid\s+moni_mslong_params_default\s*\(", hdr) and re.search(r"\bint\s+moni_ms_long_batch\s*\(", hdr)
    for name in ("moni_mslong_params_t", "moni_mslong_stats_t"):
        assert re.search(r"\}\s*%s\s*;" % name, hdr), name
    for name in ("moni_mslong_params_default", "moni_ms_long_batch"):
        assert name in capi.EXPORTS
    capi.build_lib()
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in ("moni_mslong_params_default", "moni_ms_long_batch"):
        assert hasattr(L, name), name
    assert ctypes.sizeof(capi.MslongParamsC) == 16 and ctypes.sizeof(capi.MslongStatsC) == 8 * 8 + 4 * 8


def test_defaults_and_argument_checks():
    L = capi.lib()
    p = capi.MslongParamsC(1, 2, (3, 4))
    L.moni_mslong_params_default(ctypes.byref(p))
    assert p.seg_len >= 8 and p.seg_len % 8 == 0 and list(p.reserved) == [0, 0]
    L.moni_mslong_params_default(None)                       # tolerated
    seq = np.frombuffer(b"ACGTACGT", dtype=np.uint8)
    offs = np.array([0, 8], dtype=np.uint64)
    b = capi.ReadBatchC(seq.ctypes.data, offs.ctypes.data, 1)
    out = np.zeros(8, dtype=np.uint64)
    st = capi.MslongStatsC()
    # no context, no batch, no parameters, no output
    assert L.moni_ms_long_batch(None, ctypes.byref(b), ctypes.byref(p), out.ctypes.data, out.ctypes.data, ctypes.byref(st)) == -22
    assert L.moni_ms_long_batch(None, None, ctypes.byref(p), out.ctypes.data, None, None) == -22
    assert L.moni_ms_long_batch(None, ctypes.byref(b), None, out.ctypes.data, None, None) == -22
    assert L.moni_ms_long_batch(None, ctypes.byref(b), ctypes.byref(p), None, None, None) == -22
    assert not out.any()


def test_split_alone_is_refused(exe, fa):
    r = subprocess.run([exe, "x", "-p", fa, "--split"], capture_output=True)
    assert r.returncode == 1 and b"--split belongs to --ms / --mems" in r.stderr, r.stderr
    for other in ("--pseudo-ms", "--extend", "-m"):
        r = subprocess.run([exe, "x", "-p", fa, "--split", other], capture_output=True)
        assert r.returncode == 1 and b"--split" in r.stderr, (other, r.stderr)


def test_split_options(exe, fa):
    r = subprocess.run([exe, "x", "-p", fa, "--ms", "--seg-len", "64"], capture_output=True)
    assert r.returncode == 1 and b"belong to --split" in r.stderr
    r = subprocess.run([exe, "x", "-p", fa, "--mems", "--overlap", "4"], capture_output=True)
    assert r.returncode == 1 and b"belong to --split" in r.stderr
    r = subprocess.run([exe, "x", "-p", fa, "--ms", "--split", "--seg-len", "7"], capture_output=True)
    assert r.returncode == 1 and b"at least 8" in r.stderr
    out = subprocess.check_output([exe, "idx/pref", "-p", fa, "--ms", "--split", "--seg-len", "64", "--overlap", "8", "--dry-run"]).decode()
    assert "reads=2 bases=20" in out and "Output file: %s_pref\n" % fa in out
    r = subprocess.run([exe, "-h"], capture_output=True)
    assert r.returncode == 1 and b"--split" in r.stderr and b".pointers may" in r.stderr
