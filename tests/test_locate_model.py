"""The plain-Python backward search of tests/locate_model.py (count, first BWT position, bytes matched, the capped list of positions by phi)
against brute force that shares nothing with it but the text: counting by direct search, rank order from a naive suffix array; and the surface
the feature adds (the exported symbols, the argument checks that need no device)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import locate_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def case():
    return lm.planted_case()


@pytest.fixture(scope="module")
def model(case):
    return lm.LocateModel(case[0])


@pytest.fixture(scope="module")
def rank_of(case):
    sa = lm.naive_sa(case[1])
    inv = [0] * len(sa)
    for k, x in enumerate(sa):
        inv[x] = k
    return inv


def test_case_is_what_it_claims(case):
    fi, text, pats = case
    assert 3500 <= len(text) <= 4500 and len(fi.seq_starts) == 4
    assert ord("N") in set(int(x) for x in np.unique(fi.heads))
    unit = pats[19]
    assert len(unit) == 40 and len(lm.occurrences(text, unit)) >= 9
    for k in (29, 30):                                           # the two patterns meant to die at the last and at a middle step do
        cnt, matched, _ = lm.brute(text, pats[k])
        assert cnt == 0 and matched == (39 if k == 29 else 19), (k, cnt, matched)
    assert sorted(set(len(p) for p in pats[:9])) == [1, 2, 7, 8, 9, 31, 32, 33, 150]
    assert lm.brute(text, pats[18])[0] == 1 and len(pats[18]) == 1100        # a whole sequence


@pytest.mark.parametrize("strands,max_occ", [(1, 0), (1, 3), (2, 1000), (2, 1)])
def test_model_equals_brute_force(case, model, rank_of, strands, max_occ):
    fi, text, pats = case
    res, pos, sq, so = model.batch(pats, strands, max_occ)
    lm.check_against_brute(text, pats, res, pos, sq, so, strands, max_occ, fi.seq_starts, rank_of)
    if max_occ == 3:                                             # the cap bites: the count stays exact, the list is the three highest ranks
        r = res[19]
        assert int(r["count"]) >= 9 and int(r["n_occ"]) == 3
    if max_occ == 0:
        assert len(pos) == 0 and not res["n_occ"].any() and not res["occ_off"].any()


def test_strand_1_is_the_forward_search_of_the_reverse_complement(case, model):
    fi, text, pats = case
    both = model.batch(pats, 2, 5)[0]
    fwd = model.batch([lm.revcomp(p) for p in pats], 1, 5)[0]
    for k in ("count", "sa_lo", "n_occ", "matched"):
        assert np.array_equal(both[k][1::2], fwd[k])
    assert lm.revcomp(b"acgtN") == b"NACGT"                      # lower case complements to upper case, other bytes stay
    assert int(both["count"][2 * 19 + 1]) == 0 or lm.revcomp(pats[19]) in text
    assert int(both["count"][-2]) == 0 and int(both["count"][-1]) >= 9          # the last pattern is the unit's reverse complement


def test_phi_is_the_suffix_array_predecessor(case, model, rank_of):
    text = case[1]
    sa = lm.naive_sa(text)
    for rank in range(1, len(sa), 7):
        assert model.phi(sa[rank]) == sa[rank - 1]


def test_every_suffix_length_of_a_dying_pattern(case, model):
    """matched = the longest suffix that occurs, whatever the step at which the search dies"""
    text = case[1]
    base = case[2][8]                                            # a 150-mer of the text
    for cut in range(0, 150, 11):
        p = bytearray(base)
        p[cut] = ord("X")
        got = model.search(bytes(p))
        assert got[0] == 0 and got[2] == 149 - cut


def test_abi_surface():
    from moni_align_amd import capi
    hdr = open(os.path.join(ROOT, "include", "moni_hip.h")).read()
    names = ("moni_locate_run", "moni_locate_sizes", "moni_locate_fetch", "moni_locate_batch")
    for name in names:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in capi.EXPORTS
    assert re.search(r"\bvoid\s+moni_locate_params_default\s*\(", hdr) and "moni_locate_params_default" in capi.EXPORTS
    capi.build_lib()
    L = capi.lib()
    p = capi.LocateParamsC(7, 7, (1, 1))
    L.moni_locate_params_default(ctypes.byref(p))
    assert (p.strands, p.max_occ, p.reserved[0], p.reserved[1]) == (1, 0, 0, 0)
    assert ctypes.sizeof(capi.LocateParamsC) == 16 and capi.LOCATE_RES_DTYPE == lm.RES_DTYPE
    # argument checks that need no device
    assert L.moni_locate_run(None, ctypes.byref(p)) == -22 and L.moni_locate_sizes(None, None, None) == -22
    assert L.moni_locate_fetch(None, None, None, None, None) == -22
    assert L.moni_locate_batch(None, None, ctypes.byref(p), None, None, None, None, None) == -22
    assert b"0.2" in L.moni_version()
