"""The plain-Python model of SPUMONI's pseudo-matching lengths (tests/pml_model.py, after include/ms/spumoni.hpp:356-410): it agrees with a
brute-force walk over the expanded BWT, stays below the true matching statistics, has the shape of a counter that is reset, and renders the
`.pseudo_lengths` text; and the surface the feature adds (the exported symbols)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import pml_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model(small_case):
    return pml_model.PmlModel(small_case.fi)


@pytest.fixture(scope="module")
def reads(small_case):
    return pml_model.sim_reads(small_case)


@pytest.fixture(scope="module")
def lengths(model, reads):
    return [model.query(r) for r in reads]


def brute_force(fi, pattern: bytes):
    """The generic walk of spumoni.hpp:286-352 over the BWT as a plain array: rank and select by counting, nothing shared with the model but
    the index arrays."""
    n = int(fi.n)
    starts = [int(x) for x in fi.starts]
    bwt = np.repeat(np.asarray(fi.heads), np.diff(np.asarray(fi.starts).astype(np.int64)))
    F = [int(x) for x in fi.F]
    thr_of_run = [int(x) for x in fi.thr]
    m = len(pattern)
    out = [0] * m
    pos, length = n - 1, 0
    for i in range(m):
        c = pattern[m - i - 1]
        where = np.nonzero(bwt == c)[0]                      # positions of c, increasing: select(k, c) = where[k]
        if len(where) == 0:
            length = 0
            pos = F[c]                                       # LF(pos, c) = F[c] + rank(pos, c)
        else:
            rnk = int(np.count_nonzero(bwt[:pos] == c))      # rank(pos, c)
            if pos < n and bwt[pos] == c:
                length += 1
                pos = F[c] + rnk
            else:
                thr = n + 1
                nxt = pos
                if rnk < len(where):
                    j = int(where[rnk])                      # first position of the next run of c
                    run_of_j = max(k for k in range(len(starts) - 1) if starts[k] <= j)
                    thr = thr_of_run[run_of_j]
                    nxt = j
                if pos < thr:
                    rnk -= 1
                    nxt = int(where[rnk])                    # last position of the previous run of c
                length = 0
                pos = F[c] + int(np.count_nonzero(bwt[:nxt] == c))
        out[m - i - 1] = length
    return out


def test_model_equals_brute_force(small_case, reads, lengths):
    for r, l in zip(reads, lengths):
        assert brute_force(small_case.fi, r) == l


def true_ms_length(text: bytes, r: bytes, k: int) -> int:
    lo, hi = 0, len(r) - k                                   # the longest prefix of r[k:] that occurs in the text
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if text.find(r[k:k + mid]) >= 0:
            lo = mid
        else:
            hi = mid - 1
    return lo


def test_bounded_by_matching_statistics(small_case, reads, lengths):
    text = small_case.text
    for r, l in zip(reads, lengths):
        for k in range(len(r)):
            assert l[k] <= true_ms_length(text, r, k), (k, l[k])


def test_shape(reads, lengths):
    for r, l in zip(reads, lengths):
        m = len(r)
        assert len(l) == m
        for k in range(m):
            assert l[k] == 0 or l[k] == (l[k + 1] if k + 1 < m else 0) + 1
        if m:
            assert l[m - 1] <= 1


def test_absent_letters_give_zero(small_case, model, reads, lengths):
    present = set(int(x) for x in np.unique(small_case.fi.heads))
    seen = 0
    for r, l in zip(reads, lengths):
        for k, b in enumerate(r):
            if b not in present:
                assert l[k] == 0
                seen += 1
    assert seen >= 3 + 150                                   # the NNN and the lower-case read
    assert ord("N") not in present and ord("a") not in present
    mixed = pml_model.mixed_case(small_case.text[900:1050])
    k = reads.index(mixed)
    assert max(present) < ord("a") and lengths[k][40] == 0 and lengths[k][39] == 0 and max(lengths[k]) >= 25          # position n holds no letter: a jump, and the walk goes on


def test_not_vacuous(reads, lengths):
    total = sum(len(r) for r in reads)
    long_ones = sum(1 for l in lengths for x in l if x >= 25)
    assert total >= 3000 and long_ones * 10 >= total, (long_ones, total)


def test_batch_layout(model, reads, lengths):
    flat, mx, hits = model.batch(reads, thr=25)
    assert len(flat) == sum(len(r) for r in reads) and len(mx) == len(hits) == len(reads)
    assert mx[-1] == 0 and hits[-1] == 0                     # the empty read
    assert [int(x) for x in flat[:150]] == lengths[0] and int(mx[0]) == max(lengths[0])
    assert int(hits[0]) == sum(1 for x in lengths[0] if x >= 25)


def test_renderer():
    assert pml_model.render([[45, 44, 43], [], [0]]) == b">0\n45 44 43 \n>1\n\n>2\n0 \n"
    assert pml_model.render([[1, 0]], first=7) == b">7\n1 0 \n"


def test_abi_surface():
    from moni_align_amd import capi
    hdr = open(os.path.join(ROOT, "include", "moni_hip.h")).read()
    names = ("moni_pml_run", "moni_pml_fetch", "moni_pml_batch")
    for name in names:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in capi.EXPORTS
    capi.build_lib()
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in names:
        assert hasattr(L, name), name
    assert b"0.2" in capi.lib().moni_version()
    # argument checks that need no device
    assert capi.lib().moni_pml_run(None, 25) != 0 and capi.lib().moni_pml_fetch(None, None, None, None) != 0
    assert capi.lib().moni_pml_batch(None, None, 25, None, None, None) != 0
    assert hasattr(L, "moni_pml_sizes") and capi.lib().moni_pml_sizes(None, None, None) != 0
