"""tests/approx_model.py against itself: the tree search over the r-index arrays and the sliding-window brute force agree on the planted case for
every k, both strands - counts per distance, the set of matching strings (as intervals), every position of every string; k = 0 is LocateModel's
search; the pieces change nothing but who does the work."""
import numpy as np
import pytest

from tests import approx_model as am
from tests import locate_model as lm

ALL = 1 << 30


@pytest.fixture(scope="module")
def case():
    fi, text, pats = lm.planted_case()
    return fi, text, pats, am.ApproxModel(fi)


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_model_equals_brute_force(case, k):
    fi, text, pats, model = case
    res, hits, pos, sq, so, tree, all_hits = model.approx_batch(pats, 2, k, ALL, ALL, 16, 0)
    am.check_against_brute(text, pats, res, hits, pos, sq, so, 2, k, ALL, ALL, fi.seq_starts)
    assert int(res["cnt"][:, k + 1:].sum()) == 0 and int(res["complete"].min()) == 1
    if k >= 1:                                               # hap1 is ref with a substitution every 97 bases: a 150-mer of ref occurs again at 1 or 2
        r = res[8 * 2]
        assert int(r["cnt"][0]) >= 1 and int(r["cnt"][1]) + int(r["cnt"][2]) >= 1


def test_k0_is_locate(case):
    fi, text, pats, model = case
    res, hits, pos, sq, so, tree, _ = model.approx_batch(pats, 2, 0, 1, 5, 16, 0)
    want, wpos, wsq, wso = model.batch(pats, 2, 5)
    assert np.array_equal(res["cnt"][:, 0], want["count"]) and np.array_equal(res["matched"], want["matched"])
    assert np.array_equal(res["n_hits"], (want["count"] > 0).astype(np.uint64))
    assert np.array_equal(hits["sa_lo"], want["sa_lo"][want["count"] > 0]) and np.array_equal(hits["n_occ"], want["n_occ"][want["count"] > 0])
    assert np.array_equal(pos, wpos) and np.array_equal(sq, wsq) and np.array_equal(so, wso)
    steps = sum(min(len(p), int(m) + 1) if len(p) else 0 for p, m in zip([x for p in pats for x in (p, lm.revcomp(p))], want["matched"]))
    assert tree <= steps                                     # (a byte the BWT does not hold ends the path without a step)


@pytest.mark.parametrize("k", [1, 3])
def test_pieces_change_nothing(case, k):
    fi, text, pats, model = case
    base = model.approx_batch(pats, 2, k, ALL, 3, 1 << 20, 0)
    for chunk_len in (1, 7, 16):
        got = model.approx_batch(pats, 2, k, ALL, 3, chunk_len, 0)
        for a, b in zip(got[:5], base[:5]):
            assert np.array_equal(a, b), chunk_len
        assert got[5] == base[5] and got[6] == base[6], chunk_len


def test_max_steps_gives_lower_bounds(case):
    fi, text, pats, model = case
    full = model.approx_batch(pats, 1, 2, ALL, 0, 16, 0)[0]
    cut = model.approx_batch(pats, 1, 2, ALL, 0, 16, 40)[0]
    stopped = cut["complete"] == 0
    assert stopped.any() and not stopped.all()
    assert (cut["cnt"] <= full["cnt"]).all() and (cut["n_hits"] <= full["n_hits"]).all()
    assert np.array_equal(cut["cnt"][~stopped], full["cnt"][~stopped]) and np.array_equal(cut["n_hits"][~stopped], full["n_hits"][~stopped])
    assert (cut["n_hits"][stopped] < full["n_hits"][stopped]).any()
