"""The plain-Python definition of read screening (tests/screen_model.py): its window score agrees with a sort-based statement of
the one-sided Kolmogorov-Smirnov numerator, its window rule holds at the edges, and the screen it defines is not vacuous - simulated reads of
either strand are called present, random ones absent, chimeras by their share of windows; and the surface the feature adds."""
import os
import re

import numpy as np
import pytest

from tests import pml_model, screen_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = sm.Params


def ecdf_d(a, b) -> int:
    """the largest gap #{b <= v} - #{a <= v} over every v, by sorting the clipped samples: nothing shared with screen_model.ks_d"""
    a = np.sort(np.minimum(np.asarray(a, dtype=np.int64), sm.BINS - 1))
    b = np.sort(np.minimum(np.asarray(b, dtype=np.int64), sm.BINS - 1))
    grid = np.union1d(a, b)          # the gap changes at sample values only; at the largest one both counts are len
    return int((np.searchsorted(b, grid, side="right") - np.searchsorted(a, grid, side="right")).max())


def test_ks_numerator_against_sorting():
    rng = np.random.default_rng(5)
    for _ in range(400):
        n = int(rng.integers(1, 80))
        hi = int(rng.choice([2, 8, 31, 32, 33, 200]))
        a, b = rng.integers(0, hi, size=n), rng.integers(0, hi, size=n)
        d = sm.ks_d(a, b)
        assert d == ecdf_d(a, b) and 0 <= d <= n
    for n in (1, 8, 50):
        assert sm.ks_d([7] * n, [7] * n) == 0                       # all equal
        assert sm.ks_d([40] * n, [31] * n) == 0                     # all clipped: both are BINS-1
        assert sm.ks_d([200] * n, [0] * n) == n == ecdf_d([200] * n, [0] * n)
        assert sm.ks_d([0] * n, [200] * n) == 0 == ecdf_d([0] * n, [200] * n)      # the null above the pattern: a gap below 0 reads 0
        assert sm.ks_d([30] * n, [31] * n) == 0 and sm.ks_d([31] * n, [30] * n) == n
    assert sm.ks_d([5], [5]) == 0 and sm.ks_d([5], [4]) == 1 and sm.ks_d([4], [5]) == 0      # length 1


@pytest.mark.parametrize("prm", [P(50, 25), P(64, 32), P(8, 1), P(8, 8), P(150, 75)])
def test_window_rule(prm):
    W, mw = prm.window, prm.min_win
    want = {0: 0, mw - 1: 0, mw: 1, W - 1: 1 if W - 1 >= mw else 0, W: 1, W + mw - 1: 1, W + mw: 2, 2 * W: 2}
    for m, n in want.items():
        wins = sm.windows(m, prm)
        assert len(wins) == n, (m, wins)
        assert all(hi - lo == W or (hi == m and hi - lo >= mw) for lo, hi in wins)
        assert [lo for lo, _ in wins] == [j * W for j in range(len(wins))]


def test_params_ranges():
    assert sm.params_ok(P()) and P() == (50, 25, 1, 4, 2)
    for bad in (P(window=7), P(window=65536), P(min_win=0), P(min_win=51), P(ks_num=0), P(ks_num=5), P(ks_den=65536, ks_num=1), P(strands=0), P(strands=3)):
        assert not sm.params_ok(bad), bad
    for good in (P(window=8, min_win=8), P(window=65535, min_win=1), P(ks_num=4), P(ks_num=65535, ks_den=65535), P(strands=1)):
        assert sm.params_ok(good), good


PARAM_SETS = (P(50, 25), P(64, 32), P(150, 75))


def revcomp(r: bytes) -> bytes:
    return bytes(sm.COMPL[np.frombuffer(r, dtype=np.uint8)][::-1].tolist())


def read_sets(case):
    sim = [r.tobytes() for r in case.synth.make_reads(case.pg, 300, 150, seed=5, sub_rate=0.02, indel_rate=0.003)]
    rng = np.random.default_rng(77)
    rnd = [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=150)].tobytes() for _ in range(300)]
    return sim, [revcomp(r) for r in sim[:100]], rnd


def check_not_vacuous(case):
    model = pml_model.PmlModel(case.fi)
    sim, rc, rnd = read_sets(case)
    walked = {r: sm.walk_read(model, r) for r in sim + rc + rnd}
    for prm in PARAM_SETS:
        call = lambda reads: sm.n_present([sm.screen_read(model, r, prm, walked=walked[r]) for r in reads])
        n_sim, n_rc, n_rnd = call(sim), call(rc), call(rnd)
        print("window %d/%d: simulated %d/300, reverse complements %d/100, random %d/300" % (prm.window, prm.min_win, n_sim, n_rc, n_rnd))
        assert n_sim * 100 >= 95 * 300 and n_rc * 100 >= 95 * 100 and n_rnd * 100 <= 5 * 300
    # a read and its reverse complement trade strands
    prm = P()
    for r in sim[:20]:
        a, b = sm.screen_read(model, r, prm, walked=walked[r]), sm.screen_read(model, revcomp(r), prm)
        assert a[1] == b[1][::-1] and a[2] == b[2][::-1] and a[3] == b[3][::-1] and a[0] == b[0]


def test_not_vacuous_medium(medium_case):
    check_not_vacuous(medium_case)


def test_not_vacuous_small(small_case):
    check_not_vacuous(small_case)


def chimeras(case):
    """(64 text + 64 random, 128 text + 64 random, 64 random + reverse complement of 128 text)"""
    rng = np.random.default_rng(78)
    rnd = lambda n: np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes()
    t = case.text
    return [t[1000:1064] + rnd(64), t[2000:2128] + rnd(64), rnd(64) + revcomp(t[3000:3128])]


def test_chimeras(medium_case):
    model = pml_model.PmlModel(medium_case.fi)
    prm = P(64, 32)
    half, two_thirds, minus = [sm.screen_read(model, r, prm) for r in chimeras(medium_case)]
    assert half[0] == 2 and half[1][0] == 1 and not half[4] & sm.PRESENT                      # 1 of 2 windows
    assert two_thirds[0] == 3 and two_thirds[1][0] == 2 and two_thirds[4] == sm.PRESENT
    assert minus[0] == 3 and minus[1][1] == 2 and minus[4] == sm.PRESENT | sm.STRAND1


def test_short_reads_and_one_strand(medium_case):
    model = pml_model.PmlModel(medium_case.fi)
    t = medium_case.text
    assert sm.screen_read(model, b"") == (0, (0, 0), (0, 0), (0, 0), sm.SHORT)
    short = sm.screen_read(model, t[500:524])
    assert short[0] == 0 and short[4] == sm.SHORT and 0 < short[3][0] <= 24                  # too short to score, the walk is still reported
    rc = revcomp(t[700:850])
    both, one = sm.screen_read(model, rc), sm.screen_read(model, rc, P(strands=1))
    assert both[4] == sm.PRESENT | sm.STRAND1 and one[4] == 0 and one[1][1] == one[2][1] == one[3][1] == 0
    assert (one[1][0], one[2][0], one[3][0]) == (both[1][0], both[2][0], both[3][0])
    exact = sm.screen_read(model, t[100:400])
    assert 250 < exact[3][0] <= 300 and exact[2][0] == 50 and exact[1][0] >= 5 and exact[0] == 6      # far above the clip: max_pml is not clipped, D is the window length


def test_render():
    recs = [(3, (3, 0), (50, 4), (150, 9), sm.PRESENT), (3, (0, 2), (3, 40), (8, 120), sm.PRESENT | sm.STRAND1), (3, (1, 1), (20, 20), (30, 30), 0), (0, (0, 0), (0, 0), (7, 3), sm.SHORT)]
    reads = [b"A" * 150, b"C" * 150, b"G" * 150, b"T" * 7]
    got = sm.render([b"r0", b"r1", b"r2", b"r3"], reads, recs)
    assert got == (b"r0\t150\tP\t+\t3\t3\t0\t50\t4\t150\t9\n" b"r1\t150\tP\t-\t3\t0\t2\t3\t40\t8\t120\n" b"r2\t150\tA\t.\t3\t1\t1\t20\t20\t30\t30\n"
                   b"r3\t7\tS\t.\t0\t0\t0\t0\t0\t7\t3\n")


def test_surface():
    """the header declares the family and the record is 32 bytes; capi exports it with a dtype of that size"""
    from moni_align_amd import capi
    hdr = open(os.path.join(ROOT, "include", "moni_hip.h")).read()
    for name in ("moni_screen_params_default", "moni_screen_run", "moni_screen_sizes", "moni_screen_fetch", "moni_screen_batch"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in capi.EXPORTS
    assert re.search(r"#define\s+MONI_SCREEN_BINS\s+32\b", hdr)
    assert capi.SCREEN_RES_DTYPE.itemsize == 32
    assert [f for f, _ in capi.ScreenParamsC._fields_][:5] == ["window", "min_win", "ks_num", "ks_den", "strands"]
