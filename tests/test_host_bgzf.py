"""bgzf_block (moni_align_amd/csrc/bgzf_core.h: what bgzf_block_kernel runs per BGZF block) replayed on the host, lanes as loops and phases in
launch order, against tests/bgzf_model.py and the standard library's zlib / gzip; the code-length builder against the Kraft equality.  The real
kernel is held to the replay's bytes under -m gpu (tests/test_gpu_bgzf.py)."""
import ctypes as C
import functools
import gzip
import os
import subprocess
import zlib
from fractions import Fraction

import numpy as np
import pytest

from moni_align_amd import capi
from tests import bgzf_model as bm

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sim")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SAMS = ("align_small.sam", "align_small_lifted.sam", "pe_small.sam", "pe_small_orphan.sam")
_lib = None


def sim_lib():
    """tests/host_sim/libbgzf_sim.so, built beside the host-sim library and leaving it alone"""
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "libbgzf_sim.so")
        src = os.path.join(HERE, "bgzf_sim.cpp")
        deps = [src, os.path.join(capi.CSRC, "bgzf_core.h"), os.path.join(os.path.dirname(capi.HERE), "include", "moni_hip.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
        L = C.CDLL(so)
        L.bgzfsim_compress.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(capi.BgzfParamsC), C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]
        L.bgzfsim_build_lengths.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
        L.bgzfsim_len_sym.argtypes = [C.c_uint32, C.c_void_p]
        L.bgzfsim_dist_sym.argtypes = [C.c_uint32, C.c_void_p]
        L.bgzfsim_hash3.argtypes = [C.c_char_p]
        L.bgzfsim_hash3.restype = C.c_uint32
        L.bgzfsim_crc_combine.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
        L.bgzfsim_crc_combine.restype = C.c_uint32
        _lib = L
    return _lib


STAT_KEYS = ("in_bytes", "out_bytes", "blocks", "stored_blocks", "matches", "literals", "size_mismatches")


def sim_compress(data: bytes, block_size: int = 65280, level: int = 1, eof: bool = False, reserved: int = 0, rc_only: bool = False):
    """the replay's stream and its stats (the fields of moni_bgzf_stats_t without the times; size_mismatches: blocks whose emitted bits missed
    the size computed from the histograms - always 0)"""
    p = capi.BgzfParamsC(block_size, level, 1 if eof else 0, reserved)
    nb = (len(data) + block_size - 1) // block_size if block_size else 0
    out = np.zeros(len(data) + 31 * nb + 28, dtype=np.uint8)
    buf = np.frombuffer(data, dtype=np.uint8)
    n, st = C.c_uint64(), np.zeros(7, dtype=np.uint64)
    rc = sim_lib().bgzfsim_compress(buf.ctypes.data if len(data) else None, len(data), C.byref(p), out.ctypes.data, C.byref(n), st.ctypes.data)
    if rc_only:
        return rc
    assert rc == 0, rc
    return out[:n.value].tobytes(), dict(zip(STAT_KEYS, (int(x) for x in st)))


def check(data: bytes, block_size: int = 65280, level: int = 1, eof: bool = False):
    """the properties every stream has; returns (stream, stats, walk's blocks)"""
    z, st = sim_compress(data, block_size, level, eof)
    blocks = bm.walk(z, block_size)
    assert b"".join(b for b, _ in blocks) == data
    assert (gzip.decompress(z) if z else b"") == data
    nb = (len(data) + block_size - 1) // block_size
    assert len(blocks) == nb + (1 if eof else 0) == st["blocks"]
    assert all(len(b) == block_size for b, _ in blocks[:nb - 1]), "only a batch's last block is short"
    assert st["in_bytes"] == len(data) and st["out_bytes"] == len(z) and st["size_mismatches"] == 0
    assert st["stored_blocks"] == sum(1 for _, t in blocks[:nb] if t == 0)
    assert all(t in (0, 2) for _, t in blocks[:nb])
    if level == 0:
        assert st["stored_blocks"] == nb and st["matches"] == 0 and len(z) == len(data) + 31 * nb + (28 if eof else 0)
    if eof:
        assert z.endswith(bm.EOF_BLOCK)
    return z, st, blocks


def de_bruijn_acgt3() -> bytes:
    """the linearised de Bruijn sequence B(4, 3) over ACGT: 66 bytes, every 3-mer once"""
    k, n = 4, 3
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    s = bytes(b"ACGT"[x] for x in seq + seq[:n - 1])
    assert len(s) == 66 and len({s[i:i + 3] for i in range(64)}) == 64
    return s


def unique_trigram_text(n: int, seed: int, marks) -> bytes:
    """n bytes below 48 in which no 3 bytes occur twice (under six bits a byte: a dynamic block wins), then `marks`: (position, bytes) written
    over it.  The markers use the bytes 250..255, so every repeat of the result goes through a marker; the caller asserts which 3-byte
    windows repeat.  The matcher keeps one position per hash-table slot, the latest: no other window of the text may fall into a marker's
    slot, or the marker's first occurrence would be forgotten before its second comes - the text avoids those slots (asserted by the caller)."""
    rng = np.random.default_rng(seed)
    taken = {sim_lib().bgzfsim_hash3(bytes(m)) for _, m in marks}
    out, seen = bytearray(), set()
    draws = rng.integers(0, 48, size=8 * n).tolist()
    k = 0
    while len(out) < n:
        b = draws[k]
        k += 1
        if len(out) >= 2:
            tri = (out[-2], out[-1], b)
            if tri in seen or sim_lib().bgzfsim_hash3(bytes(tri)) in taken:
                continue
            seen.add(tri)
        out.append(b)
    for at, m in marks:
        out[at:at + len(m)] = m
    return bytes(out)


def repeated_trigrams(s: bytes):
    first, rep = {}, {}
    for i in range(len(s) - 2):
        w = s[i:i + 3]
        if w in first:
            rep.setdefault(w, [first[w]]).append(i)
        else:
            first[w] = i
    return rep


@functools.lru_cache(maxsize=None)
def distance_text(d1: int = 32768, d2: int = 32769):
    """40000 bytes whose only repeats are two 3-byte markers: one again after d1 bytes, one after d2"""
    m1, m2 = bytes([250, 251, 252]), bytes([253, 254, 255])
    s = unique_trigram_text(40000, 5, ((100, m1), (100 + d1, m1), (3000, m2), (3000 + d2, m2)))
    assert repeated_trigrams(s) == {m1: [100, 100 + d1], m2: [3000, 3000 + d2]}
    slots = {sim_lib().bgzfsim_hash3(m) for m in (m1, m2)}
    assert [i for i in range(len(s) - 2) if sim_lib().bgzfsim_hash3(s[i:i + 3]) in slots] == sorted([100, 100 + d1, 3000, 3000 + d2])
    return s


def random_bytes(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def mixed_bytes(n: int, seed: int) -> bytes:
    """SAM-like letters with 0x00 and 0xFF among them"""
    return bytes(np.frombuffer(b"ACGT\x00\xff\tI", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 8, size=n)])


def golden(name: str) -> bytes:
    return open(os.path.join(GOLDEN, name), "rb").read()


def cases():
    """(name, bytes, block_size, level, eof): the inputs of the issue; tests/test_gpu_bgzf.py sends the same ones through the kernel"""
    c = [("len%d" % n, mixed_bytes(n, n), 65280, 1, n != 1) for n in (0, 1, 2)]
    c += [("de_bruijn", de_bruijn_acgt3(), 65280, 1, False), ("runs", b"A" * 1000, 65280, 1, True), ("distance", distance_text(), 65280, 1, False),
          ("random70000", random_bytes(70000, 3), 65280, 1, False), ("mixed", mixed_bytes(30000, 4), 65280, 1, True)]
    c += [(name, golden(name), 65280, 1, True) for name in SAMS]
    c += [("len%d" % n, golden("pe_small.sam")[:n], 65280, 1, False) for n in (65279, 65280, 65281)]
    c += [("pe_small/%d" % bs, golden("pe_small.sam"), bs, 1, bs == 258) for bs in (1, 3, 258, 4096)]
    c += [("level0", golden("align_small.sam"), 65280, 0, True), ("level0/4096", random_bytes(10000, 9), 4096, 0, False)]
    return c


CASES = cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_stream(case):
    _, data, bs, level, eof = case
    check(data, bs, level, eof)


def test_short_inputs():
    assert sim_compress(b"") == (b"", dict(zip(STAT_KEYS, (0, 0, 0, 0, 0, 0, 0))))
    z, st = sim_compress(b"", eof=True)
    assert z == bm.EOF_BLOCK and st["blocks"] == 1 and st["out_bytes"] == 28
    for n in (1, 2):
        z, st, blocks = check(b"AC"[:n])
        assert blocks == [(b"AC"[:n], 0)] and len(z) == n + 31


def test_no_match_and_dynamic_wins():
    """B(4, 3): no 3-mer twice, so no match and no distance code (one code of length 0 is sent); two bits a letter beat the stored block"""
    z, st, blocks = check(de_bruijn_acgt3())
    assert blocks[0][1] == 2 and st["matches"] == 0 and st["literals"] == 66 and st["stored_blocks"] == 0
    assert len(z) < 66 + 31


def test_runs_one_distance_code():
    """1000 x A: a literal, then matches at distance 1 - one distance code, sent as one code of length 1 - of length 258 while the text lasts"""
    z, st, blocks = check(b"A" * 1000)
    assert blocks[0][1] == 2 and st["literals"] == 1 and st["matches"] == 4          # 1 + 3 * 258 + 225
    assert len(z) < 80


def test_distance_limit():
    """the marker 32768 bytes back is taken, the one 32769 bytes back is not: one match in a text whose only repeats are those two"""
    s = distance_text()
    z, st, blocks = check(s)
    assert st["matches"] == 1 and st["literals"] == len(s) - 3
    # the far marker one byte nearer: both are taken; both one byte further: none is
    assert check(distance_text(32768, 32768))[1]["matches"] == 2
    assert check(distance_text(32769, 32770))[1]["matches"] == 0


def test_random_is_stored():
    data = random_bytes(70000, 3)
    z, st, blocks = check(data)
    assert [t for _, t in blocks] == [0, 0] and st["stored_blocks"] == 2 and st["out_bytes"] == len(data) + 2 * (26 + 5)


def test_many_blocks():
    data = golden("pe_small.sam")
    z, st, blocks = check(data, 258, 1, True)
    assert len(blocks) == 365 + 1


def test_block_boundaries_do_not_leak():
    """a block's bytes depend on its own text alone: the stream of a text cut at a multiple of block_size is the two streams joined"""
    data = golden("pe_small_orphan.sam")
    for bs, cut in ((65280, 65280), (4096, 5 * 4096), (258, 100 * 258)):
        whole, _ = sim_compress(data, bs)
        a, _ = sim_compress(data[:cut], bs)
        b, _ = sim_compress(data[cut:], bs)
        assert whole == a + b


@pytest.mark.parametrize("name", SAMS)
def test_compression_condition(name):
    """level 1, block_size 65280: the output, headers included, is at most the order-0 entropy of the input's blocks - Huffman coding alone
    cannot get there.  zlib level 1 cut the same way: 5531 / 5399 / 21782 / 22394 bytes."""
    data = golden(name)
    z, st = sim_compress(data)
    bound = bm.order0_bytes(data)
    print("%s: %d bytes -> %d (order-0 bound %.0f)" % (name, len(data), len(z), bound))
    assert len(z) <= bound
    assert st["matches"] > 0 and st["stored_blocks"] == 0


def test_parameter_ranges():
    for kw in (dict(block_size=0), dict(block_size=65281), dict(level=2), dict(reserved=1)):
        assert sim_compress(b"ACGT", rc_only=True, **kw) == -22, kw
    assert sim_compress(b"ACGT", rc_only=True, block_size=1) == 0 and sim_compress(b"ACGT", rc_only=True, block_size=65280, level=0) == 0


# ---- the pieces ----------------------------------------------------------------------------------------------------------------------

def build_lengths(freq, limit, complete=False):
    f = np.asarray(freq, dtype=np.uint32)
    ln, code = np.zeros(len(f), dtype=np.uint8), np.zeros(len(f), dtype=np.uint16)
    assert sim_lib().bgzfsim_build_lengths(f.ctypes.data, len(f), limit, 1 if complete else 0, ln.ctypes.data, code.ctypes.data) == 0
    return [int(x) for x in ln], [int(x) for x in code]


def kraft(lengths) -> Fraction:
    return sum(Fraction(1, 2 ** l) for l in lengths if l)


def assert_prefix_free(lengths, codes):
    """the codes as DEFLATE packs them (first bit of the code = least significant bit) are the canonical ones of RFC 1951 3.2.2"""
    want, code = {}, 0
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt = [0] * 17
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    for s, l in enumerate(lengths):
        if l:
            want[s] = int(format(nxt[l], "0%db" % l)[::-1], 2)
            nxt[l] += 1
    assert {s: c for s, c in enumerate(codes) if lengths[s]} == want


def fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def test_code_lengths():
    # Fibonacci counts: the Huffman tree is a path, 19 deep for 20 symbols and 11 for 12 - past the limits 15 and 7
    for freq, limit, pad in ((fib(20), 15, 286), (fib(12), 7, 19)):
        f = [0] * pad
        f[3:3 + len(freq)] = freq[::-1]
        ln, code = build_lengths(f, limit, complete=limit == 7)
        used = [l for l, x in zip(ln, f) if x]
        assert all(1 <= l <= limit for l in used) and max(used) == limit and kraft(ln) == 1
        assert all(l == 0 for l, x in zip(ln, f) if not x)
        assert [ln[3 + i] for i in range(len(freq))] == sorted(used), "a more frequent symbol has no longer code"
        assert_prefix_free(ln, code)
    # the same counts within the limit: the tree as it is
    ln, _ = build_lengths(fib(8), 15)
    assert sorted(ln) == [1, 2, 3, 4, 5, 6, 7, 7] and kraft(ln) == 1
    # one used symbol: one code of length 1 (RFC 1951 3.2.7, the distance code of a block with one distance) ...
    f = [0] * 30
    f[7] = 12
    ln, code = build_lengths(f, 15)
    assert ln == [0] * 7 + [1] + [0] * 22 and code[7] == 0
    # ... and in the code-length code, which inflate takes only complete, a second symbol with the other code
    for s in (0, 5):
        f = [0] * 19
        f[s] = 3
        ln, code = build_lengths(f, 7, complete=True)
        assert ln[s] == 1 and sum(ln) == 2 and kraft(ln) == 1
        assert_prefix_free(ln, code)
    # no used symbol: no code
    assert build_lengths([0] * 30, 15)[0] == [0] * 30
    # two used symbols: a bit each
    f = [0] * 286
    f[65], f[256] = 1000, 1
    ln, code = build_lengths(f, 15)
    assert ln[65] == 1 and ln[256] == 1 and sum(ln) == 2 and sorted((code[65], code[256])) == [0, 1]
    # all 286 symbols once: 226 codes of 8 bits and 60 of 9 (x + y = 286, 2 x + y = 512)
    ln, code = build_lengths([1] * 286, 15)
    assert kraft(ln) == 1 and sorted(set(ln)) == [8, 9] and ln.count(8) == 512 - 286
    assert_prefix_free(ln, code)
    # random counts: a Huffman code's cost where the limit does not bind
    rng = np.random.default_rng(11)
    for _ in range(20):
        f = (rng.integers(0, 4, size=286) * rng.integers(0, 2000, size=286)).tolist()
        f[256] = 1
        ln, code = build_lengths(f, 15)
        assert kraft(ln) == 1 and max(ln) <= 15 and all((l > 0) == (x > 0) for l, x in zip(ln, f))
        assert_prefix_free(ln, code)
        if max(huffman_depths(f)) <= 15:
            assert sum(l * x for l, x in zip(ln, f)) == huffman_cost(f)


def huffman_depths(freq):
    import heapq
    h = [(f, i, (i,)) for i, f in enumerate(freq) if f]
    depth = {i: 0 for _, i, _ in h}
    heapq.heapify(h)
    k = len(freq)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(h, (a[0] + b[0], k, a[2] + b[2]))
        k += 1
    return [depth.get(i, 0) for i in range(len(freq))]


def huffman_cost(freq):
    return sum(d * f for d, f in zip(huffman_depths(freq), freq))


def test_symbols_and_crc():
    L = sim_lib()
    # RFC 1951 3.2.5
    len_base = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    len_bits = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
    dist_base = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
    dist_bits = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
    o = np.zeros(3, dtype=np.uint32)
    for n in range(3, 259):
        L.bgzfsim_len_sym(n, o.ctypes.data)
        k = max(i for i in range(29) if len_base[i] <= n)
        assert (int(o[0]), int(o[1]), int(o[2])) == (257 + k, len_bits[k], n - len_base[k]), n
    for d in list(range(1, 2000)) + [2048, 2049, 4096, 4097, 16384, 16385, 24576, 24577, 32767, 32768]:
        L.bgzfsim_dist_sym(d, o.ctypes.data)
        k = max(i for i in range(30) if dist_base[i] <= d)
        assert (int(o[0]), int(o[1]), int(o[2])) == (k, dist_bits[k], d - dist_base[k]), d
    data = golden("align_small.sam")
    for cut in (0, 1, 7, 255, 256, 10000, len(data) - 1, len(data)):
        a, b = data[:cut], data[cut:]
        assert L.bgzfsim_crc_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(data)
