"""The plain-Python sequence counts of tests/seqcount_model.py (the interval cut at the BWT run boundaries, phi inside each piece from the run's
sample) against brute force that shares nothing with it but the text and the sequence starts; and the surface the feature adds (the exported
symbols, the defaults, the argument checks that need no device)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import locate_model as lm
from tests import seqcount_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def case():
    return lm.planted_case()


@pytest.fixture(scope="module")
def model(case):
    return sm.SeqcountModel(case[0])


@pytest.mark.parametrize("strands,max_walk", [(1, 1 << 20), (2, 1 << 20), (2, 0), (2, 8)])
def test_model_equals_brute_force(case, model, strands, max_walk):
    fi, text, pats = case
    res, counts, phi = model.seq_batch(pats, strands, max_walk)
    sm.check_against_brute(text, pats, res, counts, strands, max_walk, fi.seq_starts)
    w = res["walked"] != 0
    assert phi == int((res["count"][w].astype(np.int64) - res["n_segs"][w]).sum())
    unit = res[19 * strands]
    assert int(unit["count"]) >= 9 and int(unit["matched"]) == 40
    if max_walk == 8:                                            # the planted unit is over the limit: counted, not enumerated
        assert int(unit["walked"]) == 0 and not counts[19 * strands].any() and int((res["walked"] == 0).sum()) >= 2
    else:
        assert res["walked"].all() and int(unit["n_seqs"]) == 3 and int(counts[19 * strands].sum()) == int(unit["count"])


def test_the_segments_tile_the_interval(case, model):
    """one segment per run the interval touches; their lengths add up to the count, and the toehold of each is the suffix of its upper rank"""
    fi, text, pats = case
    sa = lm.naive_sa(text)
    seen_multi = False
    for p in pats:
        count, sa_lo, matched, toe = model.search(p)
        if not count:
            continue
        segs = model.segments(sa_lo, count, toe)
        assert sum(ln for _, ln in segs) == count
        rank = sa_lo
        for t, ln in segs:
            rank += ln
            assert sa[rank - 1] == t
        assert rank == sa_lo + count
        seen_multi |= len(segs) >= 3
    assert seen_multi


def test_abi_surface():
    from moni_align_amd import capi
    hdr = open(os.path.join(ROOT, "include", "moni_hip.h")).read()
    for name in ("moni_seqcount_run", "moni_seqcount_sizes", "moni_seqcount_fetch", "moni_seqcount_batch"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in capi.EXPORTS
    assert re.search(r"\bvoid\s+moni_seqcount_params_default\s*\(", hdr) and "moni_seqcount_params_default" in capi.EXPORTS
    capi.build_lib()
    L = capi.lib()
    p = capi.SeqcountParamsC(7, 7, 7)
    L.moni_seqcount_params_default(ctypes.byref(p))
    assert (p.strands, p.reserved, p.max_walk) == (1, 0, 1 << 20)
    assert ctypes.sizeof(capi.SeqcountParamsC) == 16 and capi.SEQCOUNT_RES_DTYPE == sm.RES_DTYPE and sm.RES_DTYPE.itemsize == 32
    # argument checks that need no device
    assert L.moni_seqcount_batch(None, None, ctypes.byref(p), None, None) == -22
    assert L.moni_seqcount_run(None, ctypes.byref(p)) == -22 and L.moni_seqcount_sizes(None, None, None) == -22
    assert L.moni_seqcount_fetch(None, None, None) == -22
