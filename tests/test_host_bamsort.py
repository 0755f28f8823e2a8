"""bam_sort_core.h (what the kernels of the coordinate sort run per record) replayed on the host, lanes as loops and passes in launch order,
against tests/bamsort_model byte for byte; every class of bad record gives its reason and the lowest index.  moni_bam_merge_plan and the
moni_bai_* builder are host-only entry points of the library: they run here through ctypes, without a GPU, against the same model.  The real
kernels are held to the replay's bytes under -m gpu (tests/test_gpu_bamsort.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from moni_align_amd import capi
from tests import bam_model as bam
from tests import bamsort_model as bsm
from tests.bamsort_cases import BAD, H1, H2, REASONS, SIZES, bad_batch, bam_file, block_sizes, cases, deflate_blocks, ents_of, offsets, record

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sim")
EINVAL = -22
_lib = None


def sim_lib():
    """tests/host_sim/libbamsort_sim.so, built beside the other host-sim libraries and leaving them alone"""
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "libbamsort_sim.so")
        src = os.path.join(HERE, "bamsort_sim.cpp")
        deps = [src, os.path.join(capi.CSRC, "bam_sort_core.h"), os.path.join(capi.CSRC, "bam_core.h"), os.path.join(capi.CSRC, "bam_index.hpp"),
                os.path.join(os.path.dirname(capi.HERE), "include", "moni_hip.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
        L = C.CDLL(so)
        L.bamsortsim_sort.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bamsortsim_gather.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32]
        L.bamsortsim_key_bits.argtypes = [C.c_uint32]
        L.bamsortsim_key_bits.restype = C.c_uint32
        _lib = L
    return _lib


def sim_sort(header: bytes, records: bytes, offs):
    """(rc, the replay's sorted records, keys, offsets, entries, stats); the buffers are exactly as large as the input says"""
    n_ref = len(bam.references(header))
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    n = len(offs) - 1
    rec = np.frombuffer(records, dtype=np.uint8)
    out, keys, oo = np.zeros(max(len(records), 1), np.uint8), np.zeros(max(n, 1), np.uint64), np.zeros(n + 1, np.uint64)
    ents, st = np.zeros(max(n, 1), capi.BAM_ENT_DTYPE), np.zeros(3, np.uint64)
    rc = sim_lib().bamsortsim_sort(n_ref, rec.ctypes.data if rec.size else None, rec.size, offs.ctypes.data, n, out.ctypes.data, keys.ctypes.data, oo.ctypes.data,
                                   ents.ctypes.data, st.ctypes.data)
    stats = dict(bad_records=int(st[0]), first_bad_record=int(st[1]), bad_reason=int(st[2]))
    if rc:
        return rc, b"", keys[:0], oo[:0], ents[:0], stats
    return rc, out[:int(oo[n])].tobytes(), keys[:n], oo, ents[:n], stats


CASES = cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_sort_equals_the_model(case):
    _, header, recs = case
    n_ref = len(bam.references(header))
    want = bsm.sort_list(n_ref, recs)
    rc, got, keys, oo, ents, st = sim_sort(header, b"".join(recs), offsets(recs))
    assert rc == 0 and st == dict(bad_records=0, first_bad_record=0, bad_reason=0)
    assert got == b"".join(want), "the replay's records differ from the model's"
    assert keys.tolist() == [bsm.key(n_ref, r) for r in want] and oo.tolist() == offsets(want).tolist()
    assert [tuple(int(x) for x in e) for e in ents] == ents_of(want)


def test_case_list_is_the_issues():
    by = {c[0]: c for c in CASES}
    assert {len(by["n%d" % n][2]) for n in (0, 1, 2, 63, 64, 65, 257)} == {0, 1, 2, 63, 64, 65, 257}
    sizes = {len(r) for c in CASES for r in c[2]}
    assert {40, 63, 64, 65, 127, 129} <= sizes and max(sizes) > 1100 and min(sizes) == 40
    assert len({bsm.key(1, r) for r in by["all_keys_equal"][2]}) == 1
    assert {bsm.key(1, r) & 1 for r in by["both_strands"][2]} == {0, 1} and len({bsm.key(1, r) >> 1 for r in by["both_strands"][2]}) == 1
    assert {-1, 2 ** 31 - 2} <= {bsm.fields(r)[1] for r in by["pos_edges"][2]} and all(bsm.fields(r)[0] == 0 for r in by["pos_edges"][2])
    refs = [bsm.fields(r)[0] for r in by["unplaced_between"][2]]
    assert -1 in refs[1:-1] and refs[0] >= 0 and refs[-1] >= 0
    assert sim_lib().bamsortsim_key_bits(1) == 34 and sim_lib().bamsortsim_key_bits(300) == 42 and sim_lib().bamsortsim_key_bits(0) == 33
    assert max(bsm.fields(r)[0] for r in by["refs_300"][2]) == 299
    n_ops = {struct_n_ops(r) for r in by["cigars"][2]}
    assert {0, 1, 70} <= n_ops
    assert len(by["random2000"][2]) == 2000 and all(name in by for name in ("align_small.sam", "align_small_lifted.sam", "pe_small.sam", "pe_small_orphan.sam"))
    # the phases of source and destination mod 16, independently, within the cases themselves
    seen = set()
    for _, h, recs in CASES:
        n_ref = len(bam.references(h))
        src = dict(zip(map(id, recs), offsets(recs)[:-1].tolist()))
        want = bsm.sort_list(n_ref, recs)
        seen |= {(src[id(r)] % 16, d % 16) for r, d in zip(want, offsets(want)[:-1].tolist())}
    assert len(seen) == 256


def struct_n_ops(rec: bytes) -> int:
    return int.from_bytes(rec[16:18], "little")


def test_gather_at_every_phase():
    """every size class from every phase of the source to every phase of the destination, in buffers sized exactly"""
    data = np.random.default_rng(5).integers(0, 256, size=1140, dtype=np.uint8)
    for size in SIZES + tuple(range(0, 40)):
        for sp in range(16):
            for dp in range(16):
                assert sim_lib().bamsortsim_gather(data.ctypes.data, size, sp, dp) == 0, (size, sp, dp)


@pytest.mark.parametrize("case", BAD, ids=[b[0] for b in BAD])
def test_bad_records(case):
    reason = REASONS.index(case[2])
    for at in (5, 0, 9):          # in the middle, first, last
        rec, off = bad_batch(case, at)
        rc, got, _, _, _, st = sim_sort(H1, rec, off)
        assert rc == EINVAL and got == b""
        assert (st["first_bad_record"], st["bad_reason"]) == (at, reason), st
        assert st["bad_records"] == (1 if case[1] is not None or at == 9 else 2)          # an offset that does not move spoils the record behind it too
    # alone
    rec, off = bad_batch(case, 0)
    n0 = int(off[1]) if case[1] is not None else len(record(pos=0, ops=[(4, "M")], size=48))
    rc, _, _, _, _, st = sim_sort(H1, rec[:n0], np.array([0, 0 if case[1] is None else n0], np.uint64))
    assert rc == EINVAL and (st["bad_records"], st["first_bad_record"], st["bad_reason"]) == (1, 0, reason)


def test_two_bad_records_the_first_counts():
    """the replay takes the records last to first, so the later bad record is met first: the index is the minimum, the reason that record's"""
    for a, b in zip(BAD, BAD[1:] + BAD[:1]):
        rec, off = bad_batch(a, 2, b, 8)
        rc, _, _, _, _, st = sim_sort(H1, rec, off)
        assert rc == EINVAL and (st["first_bad_record"], st["bad_reason"]) == (2, REASONS.index(a[2])) and st["bad_records"] >= 2


# ---- moni_bam_merge_plan through ctypes ------------------------------------------------------------------------------------------------------

def _runs(lengths, seed, n_keys=50, equal=False):
    """sorted runs of records of unequal sizes: ([keys], [offs], [[records]])"""
    rng = np.random.default_rng(seed)
    runs = []
    for r, n in enumerate(lengths):
        recs = [record(ref=0, pos=5 if equal else int(rng.integers(0, n_keys)), flag=0 if equal else 16 * int(rng.integers(0, 2)), size=int(rng.integers(40, 400)), seed=1000 * r + i)
                for i in range(n)]
        runs.append(bsm.sort_list(1, recs))
    return [np.array([bsm.key(1, x) for x in run], np.uint64) for run in runs], [offsets(run) for run in runs], runs


PLANS = [("one_run", (300,), {}), ("two_runs", (120, 45), {}), ("seven_runs", (90, 5, 0, 200, 33, 1, 64), {}), ("empty_run_first", (0, 50), {}),
         ("all_empty", (0, 0), {}), ("all_keys_equal", (70, 30, 50), dict(equal=True)), ("few_keys", (200, 150, 100), dict(n_keys=3))]


@pytest.mark.parametrize("plan", PLANS, ids=[p[0] for p in PLANS])
@pytest.mark.parametrize("chunk_bytes", (1, 39, 1000, 4096, 1 << 40))
def test_merge_plan(plan, chunk_bytes):
    _, lengths, kw = plan
    keys, offs, runs = _runs(lengths, 7, **kw)
    cuts = capi.bam_merge_plan(keys, offs, chunk_bytes)
    R = len(lengths)
    assert cuts.shape[1] == R and cuts[0].tolist() == [0] * R and cuts[-1].tolist() == list(lengths)
    assert (np.diff(cuts.astype(np.int64), axis=0) >= 0).all()
    want = bsm.sort_list(1, [x for run in runs for x in run])          # the global order: stable over the runs in run order
    got = []
    for k in range(len(cuts) - 1):
        part = [x for r in range(R) for x in runs[r][int(cuts[k][r]):int(cuts[k + 1][r])]]
        size = sum(len(x) for x in part)
        assert part and (size <= chunk_bytes or len(part) == 1), "chunk %d: %d bytes in %d records" % (k, size, len(part))
        got += bsm.sort_list(1, part)
    assert got == want
    if chunk_bytes >= 1 << 40:
        assert len(cuts) - 1 == (1 if sum(lengths) else 0)
    if chunk_bytes < 40:
        assert len(cuts) - 1 == sum(lengths)          # every record is larger than the chunk: one each
    if chunk_bytes == 4096 and sum(lengths) > 100:          # chunks are filled, not merely bounded: none but the last leaves room for its successor's first record
        sizes = [sum(len(x) for r in range(R) for x in runs[r][int(cuts[k][r]):int(cuts[k + 1][r])]) for k in range(len(cuts) - 1)]
        assert all(s > 4096 - 400 for s in sizes[:-1])


def test_merge_plan_refuses_unsorted_runs():
    with pytest.raises(RuntimeError):
        capi.bam_merge_plan([np.array([2, 1], np.uint64)], [np.array([0, 40, 80], np.uint64)], 100)
    with pytest.raises(RuntimeError):
        capi.bam_merge_plan([np.array([1, 2], np.uint64)], [np.array([0, 40, 40], np.uint64)], 100)


# ---- moni_bai_* through ctypes ---------------------------------------------------------------------------------------------------------------

def _bai_of(header, recs, block_size, chunk_ends):
    data, chunks = bam_file(header, recs, block_size, chunk_ends)
    b = capi.BaiBuilder(len(bam.references(header)))
    for a, e, raw, file_off in chunks:
        b.add(np.array(ents_of(recs[a:e]), dtype=capi.BAM_ENT_DTYPE), len(raw), block_size, block_sizes(deflate_blocks(raw, block_size)), file_off)
    out = b.finish(len(data) - 28)
    b.close()
    return out, data


def test_bai_equals_the_model():
    recs = bsm.sort_list(2, cases()[-1][2])          # random2000 under H2: two references, unplaced records, both strands
    for block_size, chunk_ends in ((1000, ()), (300, (100, 700, 701, 1500)), (65280, (1000,))):
        got, data = _bai_of(H2, recs, block_size, chunk_ends)
        assert got == bsm.bai_build(data, block_size), (block_size, chunk_ends)
        for ref, beg, end in ((0, 0, 100), (0, 1500, 1600), (1, 2990, 3200), (1, 0, 1 << 29), (0, 5000, 6000)):
            assert bsm.bai_query(got, data, ref, beg, end, block_size) == bsm.brute_query(data, ref, beg, end, block_size)


def test_bai_block_and_chunk_ends():
    """records that straddle a block, that end exactly on a block's end, and that end exactly on a chunk's end (which is a block's too)"""
    recs = [record(pos=10 * i, ops=[(5, "M")], size=100, seed=i) for i in range(10)] + [record(pos=200 + i, ops=[(5, "M")], size=130, seed=i) for i in range(10)]
    recs += [record(ref=1, pos=16380 + i, ops=[(9, "M")], size=100, seed=i) for i in range(10)] + [record(ref=-1, pos=-1, size=100, seed=i) for i in range(3)]
    for block_size, chunk_ends in ((250, ()), (500, (5,)), (1000, (10, 20)), (300, (3, 30))):
        got, data = _bai_of(H2, recs, block_size, chunk_ends)
        assert got == bsm.bai_build(data, block_size), (block_size, chunk_ends)
    got, data = _bai_of(H2, [], 300, ())
    assert got == bsm.bai_build(data, 300) == b"BAI\x01" + bytes([2]) + bytes(3 + 16 + 8)


def test_bai_refuses():
    e = np.array(ents_of([record(pos=5, size=50), record(pos=4, size=50)]), dtype=capi.BAM_ENT_DTYPE)
    for ents, chunk_len, cs in ((e, 100, [60]), (e[:1], 50, [60, 60]), (e[1:], 40, [60])):          # out of order; blocks that do not fit; an offset past the chunk
        b = capi.BaiBuilder(1)
        with pytest.raises(RuntimeError):
            b.add(ents, chunk_len, 1000, cs, 0)
        b.close()
    b = capi.BaiBuilder(1)
    b.add(e[:1], 50, 1000, [60], 100)
    with pytest.raises(RuntimeError):
        b.add(e[:1], 50, 1000, [60], 170)          # a gap behind the first chunk
    b.close()
