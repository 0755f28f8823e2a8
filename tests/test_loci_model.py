"""The plain-Python reference loci of tests/loci_model.py (backward search, the interval cut at the BWT run boundaries, phi inside each piece, the
lift from the flat index's ins / del column lists, the fold) against brute force that shares nothing with it but the text: start positions by
direct search, the haplotype-to-reference map walked from the pangenome's variant lists, a Counter.  And the surface the feature adds (the exported
symbols, the defaults, the argument checks that need no device)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import locate_model as lm
from tests import loci_model as lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lifted():
    pg, fi, text, pats = lo.lifted_case()
    return pg, fi, text, pats, lo.LociModel(fi), lo.text_to_ref(pg)


def test_the_lifted_case_is_what_it_is_meant_to_be(lifted):
    pg, fi, text, pats, model, keymap = lifted
    kinds = np.concatenate([v[1] for v in pg.variants])
    assert (kinds == 0).any() and (kinds == 1).any() and (kinds == 2).any()          # SNPs, insertions and deletions
    n_seq = len(pg.seqs)
    count, _, loci = lo.brute_loci(text, b"A", keymap)
    assert (count, len(loci), max(s for _, s in loci)) == (9125, 1527, 8) and max(s for _, s in loci) > n_seq          # an insertion folded
    count, _, loci = lo.brute_loci(text, b"ACG", keymap)
    assert (count, len(loci)) == (677, 114)
    count, _, loci = lo.brute_loci(text, pats[2], keymap)                            # a 32-mer of the reference away from a site
    assert count == n_seq and loci == [(1000, n_seq)] and len(pats[2]) == 32
    count, _, loci = lo.brute_loci(text, pats[3], keymap)                            # a 20-mer that starts inside haplotype 1's insertion before base 2784
    assert len(pats[3]) == 20 and count >= 1 and dict(loci).get(2784, 0) >= 1
    at = int(pg.seq_starts[1]) + lo.inside_insertion(pg)
    assert text[at:at + 20] == pats[3] and model.lift(at) == 2784 and int(keymap[at]) == 2784


def test_the_model_lift_equals_the_variant_walk(lifted):
    """every text position outside the separators, not only those a pattern hits"""
    pg, fi, text, pats, model, keymap = lifted
    for p in range(len(keymap)):
        if keymap[p] >= 0:
            assert model.lift(p) == int(keymap[p]), p


@pytest.mark.parametrize("strands", [1, 2])
@pytest.mark.parametrize("lift", [1, 0])
def test_model_equals_brute_force_lifted(lifted, strands, lift):
    pg, fi, text, pats, model, keymap = lifted
    out = model.loci_batch(pats, strands, lift)
    n = lo.check_against_brute(text, pats, out, strands, 1 << 20, fi.seq_starts, keymap if lift else None)
    res = out[0]
    w = res["walked"] != 0
    assert out[5] == int((res["count"][w].astype(np.int64) - res["n_segs"][w]).sum()) and n == int(res["n_loci"].sum())
    if not lift:                                                 # the full locate in text order: every support is 1
        assert (out[4] == 1).all() and n == int(res["count"].sum())
        for t, r in enumerate(res):
            a, k = int(r["loci_off"]), int(r["n_loci"])
            q = lm.revcomp(pats[t // strands]) if t % strands else pats[t // strands]
            assert [int(x) for x in out[1][a:a + k]] == lm.occurrences(text, q)


def test_max_walk(lifted):
    pg, fi, text, pats, model, keymap = lifted
    out = model.loci_batch(pats, 2, 1, 8)
    lo.check_against_brute(text, pats, out, 2, 8, fi.seq_starts, keymap)
    assert int(out[0]["walked"][0]) == 0 and int(out[0]["n_loci"][0]) == 0 and 0 < int(out[0]["walked"].sum()) < len(out[0])


def test_null_lifts_lift_to_the_position_itself():
    """the FASTA-built form of the same text: lift = 1 equals lift = 0"""
    pg, fi, text, pats = lo.lifted_case(lifted=False)
    assert fi.lifts is None
    model = lo.LociModel(fi)
    a, b = model.loci_batch(pats, 2, 1), model.loci_batch(pats, 2, 0)
    assert all(np.array_equal(x, y) for x, y in zip(a[:5], b[:5])) and a[5] == b[5]
    lo.check_against_brute(text, pats, a, 2, 1 << 20, fi.seq_starts, None)
    assert (a[4] == 1).all()


@pytest.mark.parametrize("lift", [1, 0])
def test_planted_case_unlifted(lift):
    fi, text, pats = lm.planted_case()
    pats = [p for p in pats if all(c > 5 for c in p)] + [b"A", b"N"]          # (a separator byte in a pattern: its occurrences are the separators')
    out = lo.LociModel(fi).loci_batch(pats, 2, lift)
    lo.check_against_brute(text, pats, out, 2, 1 << 20, fi.seq_starts, None)
    assert (out[4] == 1).all()


def test_abi_surface():
    from moni_align_amd import capi
    hdr = open(os.path.join(ROOT, "include", "moni_hip.h")).read()
    for name in ("moni_loci_run", "moni_loci_sizes", "moni_loci_fetch", "moni_loci_batch"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in capi.EXPORTS
    assert re.search(r"\bvoid\s+moni_loci_params_default\s*\(", hdr) and "moni_loci_params_default" in capi.EXPORTS
    capi.build_lib()
    L = capi.lib()
    p = capi.LociParamsC(7, 7, 7, 7, (ctypes.c_uint64 * 2)(7, 7))
    L.moni_loci_params_default(ctypes.byref(p))
    assert (p.strands, p.lift, p.max_walk, p.max_total, p.reserved[0], p.reserved[1]) == (1, 1, 1 << 20, 1 << 28, 0, 0)
    assert ctypes.sizeof(capi.LociParamsC) == 40 and capi.LOCI_RES_DTYPE == lo.RES_DTYPE and lo.RES_DTYPE.itemsize == 48
    # argument checks that need no device
    assert L.moni_loci_batch(None, None, ctypes.byref(p), None, None, None, None, None, None) == -22
    assert L.moni_loci_run(None, ctypes.byref(p)) == -22 and L.moni_loci_sizes(None, None, None) == -22
    assert L.moni_loci_fetch(None, None, None, None, None, None) == -22
