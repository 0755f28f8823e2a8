"""bamin_core.h (what the kernels of the BAM reader run per segment and per record) replayed on the host by tests/host_sim/bamin_sim.cpp, against
tests/bamin_model.py: the texts, the counts of every call, and for damaged streams the lowest bad record and its reason.  The kernels are held
to the same under -m gpu (tests/test_gpu_bamin.py).  The replay is also built as a stand-alone program under ASan and UBSan and run over the
same streams and over damaged copies of them; no sanitizer run of code loaded into Python is made."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from moni_align_amd import capi
from tests import bamin_cases as bc
from tests import bamin_model as bm

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sim")
EINVAL = -22
SRC = os.path.join(HERE, "bamin_sim.cpp")
DEPS = [SRC] + [os.path.join(capi.CSRC, f) for f in ("bamin_core.h", "bam_sort_core.h", "bam_core.h")] + [os.path.join(os.path.dirname(capi.HERE), "include", "moni_hip.h")]
STAT_KEYS = ("records", "reads", "skipped_secondary", "skipped_empty", "carried_bytes", "bad_records", "first_bad_record", "bad_record_reason", "header_done")
_lib = None


def stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS)


def sim_lib():
    """tests/host_sim/libbamin_sim.so, built beside the other replays and leaving them alone"""
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "libbamin_sim.so")
        if stale(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
        L = C.CDLL(so)
        L.baminsim_create.restype = C.c_void_p
        L.baminsim_create.argtypes = [C.c_uint32, C.c_uint64]
        L.baminsim_destroy.argtypes = [C.c_void_p]
        L.baminsim_reset.argtypes = [C.c_void_p]
        L.baminsim_segment.restype = C.c_uint32
        L.baminsim_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int] + [C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)] * 2 + [C.POINTER(C.c_uint64), C.c_void_p]
        _lib = L
    return _lib


def segment() -> int:
    return int(sim_lib().baminsim_segment())


class Sim:
    def __init__(self, paired=False, group=0):
        self.h = sim_lib().baminsim_create(1 if paired else 0, group)

    def feed(self, data: bytes, last: bool):
        """(return code, text1, text2, reads or pairs, stats: STAT_KEYS)"""
        buf = np.frombuffer(data, dtype=np.uint8)
        t1, t2, n1, n2, nr, st = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_uint64(), np.zeros(9, dtype=np.uint64)
        rc = sim_lib().baminsim_feed(self.h, buf.ctypes.data if len(data) else None, len(data), int(last), C.byref(t1), C.byref(n1), C.byref(t2), C.byref(n2), C.byref(nr),
                                     st.ctypes.data)
        return rc, C.string_at(t1.value, n1.value) if n1.value else b"", C.string_at(t2.value, n2.value) if n2.value else b"", nr.value, dict(zip(STAT_KEYS, (int(x) for x in st)))

    def reset(self):
        sim_lib().baminsim_reset(self.h)

    def close(self):
        sim_lib().baminsim_destroy(self.h)
        self.h = None


def run_feeder(feeder, raw, paired, member, per_call):
    """bamin_cases.model_run's answer from something with feed(data, last) -> (rc, text1, text2, n_reads, stats)"""
    t1, t2, calls = [], [], []
    parts = bc.chunks(raw, member, per_call)
    for k, part in enumerate(parts):
        rc, a, b, nr, st = feeder(part, k + 1 == len(parts))
        if rc:
            assert rc == EINVAL and a == b"" and b == b"" and nr == 0 and st["bad_records"] == 1
            return ("bad", st["first_bad_record"], st["bad_record_reason"], k)
        assert st["bad_records"] == 0 and nr == (st["reads"] // 2 if paired else st["reads"]) and a.count(b"\n") == 4 * nr and b.count(b"\n") == (4 * nr if paired else 0)
        t1.append(a)
        t2.append(b)
        calls.append({k: st[k] for k in ("records", "reads", "skipped_secondary", "skipped_empty", "carried_bytes", "header_done")})
    return ("ok", b"".join(t1), b"".join(t2), calls)


def sim_run(raw, paired, member, per_call, group=0):
    s = Sim(paired, group)
    try:
        return run_feeder(s.feed, raw, paired, member, per_call)
    finally:
        s.close()


CASES = bc.cases(segment())
BAD = bc.bad_cases(segment())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_replay_equals_model(case):
    _, raw, paired, member, per_call = case
    want = bc.model_run(raw, paired, member, per_call)
    assert want[0] == "ok"
    assert sim_run(raw, paired, member, per_call) == want


def test_calls_of_any_size_give_one_text():
    by_raw = {}
    for name, raw, paired, member, per_call in CASES:
        if name.startswith(("members_", "pairs_", "decoys")):
            by_raw.setdefault((raw, paired), set()).add(bc.model_run(raw, paired, member, per_call)[1:3])
    assert len(by_raw) == 7 and all(len(v) == 1 for v in by_raw.values())


@pytest.mark.parametrize("case", BAD, ids=[c[0] for c in BAD])
def test_damaged_stream(case):
    _, raw, paired, member, per_call, index, reason = case
    want = bc.model_run(raw, paired, member, per_call)
    assert want[:3] == ("bad", index, reason)
    assert sim_run(raw, paired, member, per_call) == want


def test_group_edges():
    """groups of one, two and three segments: the chain's state passes from launch to launch"""
    for name in ("longer_than_2S", "decoys", "starts_at_S", "block_size_across_S_2"):
        _, raw, paired, member, per_call = [c for c in CASES if c[0] == name][0]
        want = bc.model_run(raw, paired, member, per_call)
        for group in (1, 2, 3):
            assert sim_run(raw, paired, member, per_call, group) == want


def test_a_refused_call_leaves_the_stream_alone_and_reset_forgets_it():
    raw = bc.HDR + bc.pair(0, 30, 31) + bc.read(7, 30, 0, 0x4D, b"lone")
    s = Sim(True)
    try:
        rc, _, _, _, st = s.feed(raw, True)
        assert rc == EINVAL and (st["first_bad_record"], st["bad_record_reason"]) == (2, bm.TRUNCATED)
        rc, a, b, nr, st = s.feed(raw, False)          # the same bytes as a first call: nothing was kept from the refused one
        assert rc == 0 and nr == 1 and st["records"] == 2 and st["carried_bytes"] == len(bc.read(7, 30, 0, 0x4D, b"lone"))
        rc, a, b, nr, st = s.feed(bc.read(8, 31, 0, 0x8D, b"lone"), True)
        assert rc == 0 and nr == 1 and a.startswith(b"@lone\n") and b.startswith(b"@lone\n") and st["carried_bytes"] == 0
        rc, _, _, _, st = s.feed(bytes([5]) + bytes(40), False)
        assert rc == EINVAL and (st["first_bad_record"], st["bad_record_reason"]) == (4, bm.BLOCK_SIZE)
        s.reset()
        rc, a, b, nr, st = s.feed(raw[:-3], False)
        assert rc == 0 and nr == 1 and st["header_done"] == 1 and st["records"] == 2
        assert s.feed(b"", False)[0] == 0 and s.feed(b"", False)[4]["carried_bytes"] == st["carried_bytes"]
    finally:
        s.close()


def write_case(d, name, raw, paired, member, per_call, group=0):
    want = bc.model_run(raw, paired, member, per_call)
    path = os.path.join(d, name)
    with open(path, "wb") as f:
        f.write(raw)
    with open(path + ".meta", "w") as f:
        f.write("%d %d %d %d %d %d\n" % ((int(paired), member * per_call, group) + ((0, 0, 0) if want[0] == "ok" else (EINVAL, want[1], want[2]))))
    if want[0] == "ok":
        for ext, t in ((".t1", want[1]), (".t2", want[2])):
            with open(path + ext, "wb") as f:
                f.write(t)
    return path


def test_sanitized_replay(tmp_path):
    """The stand-alone replay under ASan + UBSan, its buffers sized exactly: every case, every damaged stream, and copies of the small cases with
    a bit flipped, a byte dropped, the stream cut.  Each copy is refused as the model refuses it or gives the model's text."""
    exe = os.path.join(HERE, "bamin_sim_asan")
    if stale(exe):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DBAMIN_SIM_MAIN", "-o", exe, SRC])
    d, paths = str(tmp_path), []
    for i, (name, raw, paired, member, per_call) in enumerate(CASES):
        paths.append(write_case(d, "c%d" % i, raw, paired, member, per_call, group=2 if "S" in name else 0))
    for i, c in enumerate(BAD):
        paths.append(write_case(d, "b%d" % i, *c[1:5]))
    rng = np.random.default_rng(5)
    k = 0
    for name, raw, paired, member, per_call in CASES:
        if len(raw) > 4000:
            continue
        for at in range(0, len(raw), 1 + len(raw) // 40):
            flipped = raw[:at] + bytes([raw[at] ^ (1 << int(rng.integers(0, 8)))]) + raw[at + 1:]
            for copy in (flipped, raw[:at] + raw[at + 1:], raw[:at]):
                paths.append(write_case(d, "d%d" % k, copy, paired, member, per_call))
                k += 1
    assert k > 2900          # (2967 with the cases as they stand)
    for lo in range(0, len(paths), 500):
        r = subprocess.run([exe] + paths[lo:lo + 500], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
