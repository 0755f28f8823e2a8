// chain_core.h - the arithmetic of one predecessor in the chaining DP (chain.hpp:300-345), for host and device alike.
//
// cc_gain<I> is what anchor j adds to a chain that anchor i continues, alpha - beta, once the mate test and the reference-distance test
// (x_i <= x_j + max_dist_x) have passed.  I is the integer the differences are held in:
//   I = long long   the wide form: the reference's own arithmetic, for any parameters;
//   I = int32_t     the narrow form: the same values wherever cc_narrow_ok(P) holds (below), at half the registers and without the
//                   12-instruction f64 -> i64 conversion of the GPU.
// The reference ends x themselves are 40 bits and are never narrowed: only x_d = x_i - x_j is, after the test that bounds it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CC_HD __host__ __device__ __forceinline__
#else
#define CC_HD inline
#endif

#define CC_MAX_READ 512                      // a read is shorter than this: read positions and seed lengths lie in [0, CC_MAX_READ)
#define CC_NARROW_MAX_DIST (1ll << 28)       // cc_narrow_ok: the largest max_dist_x / max_dist_y
#define CC_NARROW_MAX_COUNT (1ll << 30)      // cc_narrow_ok: the largest max_iter / max_pred

CC_HD uint32_t cc_ilog2(uint32_t v) {      // floor(log2 v), v > 0
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)(31 - __clz((int)v));
#else
    return (uint32_t)(31 - __builtin_clz(v));
#endif
}

// The narrow form is exact when no intermediate leaves 32 bits.  With 0 <= max_dist_x <= 2^28, seed lengths w in [0, 512), the average seed length
// in (0, 512] and read positions y in [0, 1024) (a pair's second mate is placed behind the first: y < 2 * CC_MAX_READ):
//   x_d = x_i - x_j                 in [0, max_dist_x]: the anchors are sorted by x and the distance test has passed;
//   y_d = y_i - y_j                 in (-1024, 1024);
//   l = |y_d - x_d|                 <= 2^28 + 1023: the subtraction stays below 2^29 in magnitude;
//   .01 * l * avg                   <= .01 * (2^28 + 1023) * 512 < 1.38e9 < 2^31: the conversion of the double to int32_t truncates the same value that
//                                   the conversion to long long truncates (and the reference's own c_lin is an int already);
//   beta                            <= (1.38e9 + 31) / 2; alpha = min(x_d, y_d, w_i) in (-1024, 512);
//   score = f[j] + alpha - beta     f is a chain's score: at least the anchor's own length (> 0) and at most the sum of the lengths of a read's anchors,
//                                   < 2048 * 512 = 2^20 for the largest LDS instance, so the sum lies in (-2^30, 2^21).
// max_dist_y is only compared with y_d: any value in [-2^28, 2^28] converts.  max_iter and max_pred are compared with anchor counts, as size_t in the
// reference: a negative value means "no limit" there, which the narrow form's int32_t comparison would not give, so they must lie in [0, 2^30].
// One above any of these bounds the wide form runs: the bounds are chosen round, not tight.
template <class P>
inline bool cc_narrow_ok(const P& p) {
    return p.max_dist_x >= 0 && p.max_dist_x <= CC_NARROW_MAX_DIST && p.max_dist_y >= -CC_NARROW_MAX_DIST && p.max_dist_y <= CC_NARROW_MAX_DIST
        && p.max_iter >= 0 && p.max_iter <= CC_NARROW_MAX_COUNT && p.max_pred >= 0 && p.max_pred <= CC_NARROW_MAX_COUNT;
}

// false: the pair is skipped (same mate and j not strictly left of i in the read, or too far apart in it); true: gain = alpha - beta
template <class I>
CC_HD bool cc_gain(I x_d, I y_i, I y_j, I w_i, bool same_mate, I max_dist_y, float avg_mem_length, I& gain) {
    const I y_d = y_i - y_j;
    const int32_t l = (int32_t)(y_d > x_d ? (y_d - x_d) : (x_d - y_d));
    const uint32_t ilog_l = l > 0 ? cc_ilog2((uint32_t)l) : 0;
    if (same_mate && (y_j >= y_i || y_d > max_dist_y)) return false;
    const I mn = y_d < x_d ? y_d : x_d;
    const I alpha = mn < w_i ? mn : w_i;
    I beta = 0;
    if (!same_mate) {
        if (x_d == 0) ++beta;
        else { const int c_lin = (int)(l * .01 * avg_mem_length); beta = c_lin < (I)ilog_l ? (I)c_lin : (I)ilog_l; }
    } else {
        beta = l > 0 ? ((I)(.01 * l * avg_mem_length) + (I)ilog_l) >> 1 : 0;
    }
    gain = alpha - beta;
    return true;
}

// ------------------------------------------------------------------------------------------------------------------------------
// The chaining of ONE run of the sorted anchors (chain.hpp:278-400), for host and device alike.  A run is a maximal stretch of the sorted anchors whose
// consecutive reference ends are at most max_dist_x apart: pairs from different runs never pass the distance test, so a run's f / msc / p / t depend on
// nothing outside it, and the lower bound lb and max_iter work on index differences, which are the same run by run.
//
// S is the storage of the run.  Nodes are addressed by their place k in the run, 0 <= k < n; the VALUES of p and t are GLOBAL anchor indices (fb + k, fb the
// run's first anchor in the read; p = -1: no predecessor), because the reference compares them as such: `if (p[j] > 0) t[p[j]] = i` skips anchor 0 of the
// read, not the first anchor of every run, and `t[j] == i` meets the zero that t starts from only at the read's anchor 0.
//   x(k)                  reference end, or any value with the same differences inside the run (long long)
//   y(k), w(k), mate(k)   read position, seed length, mem_t::mate
//   f(k) msc(k) p(k) t(k) and set_f(k, v) set_msc(k, v) set_p(k, v) set_t(k, v)
// avg_mem_length is the READ's, the float the reference computes over all its anchors.
// NOTE: chain_plan_kernel's in-place path (af_chain_run and the `track` lambda of af_chain, align_fast.hip) is a second, older copy of this code over the
// wave's LDS arrays, with the second track of -Z in it.  It was deliberately not moved onto these routines (its instance sits at 64 VGPRs with spills: every
// change of its code moves them); the host simulation checks THESE routines only.  Whoever changes one copy changes the other.

// chain.hpp:278-362.  t(k) must be 0 for every node on entry.  I / U as cc_gain's: the integers of the differences, scores and indices / of the counts.
template <class I, class U, class S>
CC_HD void cc_run_dp(S& s, uint32_t fb, uint32_t n, I max_iter, U max_pred, long long max_dist_x, I max_dist_y, float avg_mem_length) {
    I lb = (I)fb;
    for (uint32_t i = fb; i < fb + n; ++i) {
        const uint32_t ki = i - fb;
        const long long x_i = s.x(ki);
        const I y_i = (I)s.y(ki), w_i = (I)s.w(ki);
        const uint32_t mate_i = s.mate(ki);
        I max_f = w_i, max_j = -1;
        U n_pred = 0;
        if ((U)i - (U)lb > (U)max_iter) lb = (I)i - max_iter;
        for (I j = (I)i - 1; j >= lb; --j) {
            const uint32_t kj = (uint32_t)j - fb;
            const long long x_j = s.x(kj);
            const uint32_t mate_j = s.mate(kj);
            if (mate_i != mate_j && ((mate_i ^ mate_j) != 3)) continue;
            if (x_i > x_j + max_dist_x) { lb = j; continue; }
            I gain;
            if (!cc_gain<I>((I)(x_i - x_j), y_i, (I)s.y(kj), w_i, mate_i == mate_j, max_dist_y, avg_mem_length, gain)) continue;
            const I score = (I)s.f(kj) + gain;
            if (score > max_f) { max_f = score; max_j = j; if (n_pred > 0) --n_pred; }
            else if ((U)(I)s.t(kj) == (U)i && (++n_pred > max_pred)) break;
            const I pj = (I)s.p(kj);
            if (pj > 0) s.set_t((uint32_t)pj - fb, (I)i);          // (global numbers: see above)
        }
        s.set_f(ki, max_f); s.set_p(ki, max_j);
        I m = max_f;
        if (max_j >= 0) { const I mp = (I)s.msc((uint32_t)max_j - fb); if (mp > max_f) m = mp; }
        s.set_msc(ki, m);
    }
}

// chain.hpp:363-378: the chain ends of the run (no successor, msc above min_chain_score) in index order, each walked back to the anchor where its best
// prefix ends; emit(j) gets that anchor's global index (its score is f of it; two ends may give the same one).  Leaves t as marks.  Returns their number.
template <class S, class Emit>
CC_HD uint32_t cc_run_starts(S& s, uint32_t fb, uint32_t n, long long min_chain_score, Emit emit) {
    for (uint32_t k = 0; k < n; ++k) s.set_t(k, 0);
    for (uint32_t k = 0; k < n; ++k) { const int pk = (int)s.p(k); if (pk >= 0) s.set_t((uint32_t)pk - fb, 1); }
    uint32_t ns = 0;
    for (uint32_t k = 0; k < n; ++k) {
        if (s.t(k) != 0 || !((long long)s.msc(k) > min_chain_score)) continue;
        uint32_t j = k;
        while (s.f(j) < s.msc(j)) j = (uint32_t)s.p(j) - fb;
        emit(fb + j);
        ++ns;
    }
    return ns;
}

// the order the starts are backtracked in, std::greater<pair<score, index>> (chain.hpp:380): does (fa, ja) come before (fb, jb)?
CC_HD bool cc_start_before(long long fa, uint32_t ja, long long fb, uint32_t jb) { return fa > fb || (fa == fb && ja > jb); }

// chain.hpp:166-200: the chain of one start (global index j0), to be called for the starts of the run in cc_start_before's order with t(k) = 0 for every node
// before the first.  visit(j) gets the chain's anchors right to left (global indices).  Returns their number; keep: the chain passes the keep test.
template <class S, class Visit>
CC_HD uint32_t cc_run_backtrack(S& s, uint32_t fb, uint32_t j0, long long min_chain_score, long long min_chain_length, bool& keep, Visit visit) {
    const long long f0 = (long long)s.f(j0 - fb);
    int j = (int)j0;
    uint32_t cnt = 0;
    do { visit((uint32_t)j); ++cnt; s.set_t((uint32_t)j - fb, 1); j = (int)s.p((uint32_t)j - fb); } while (j >= 0 && s.t((uint32_t)j - fb) == 0);
    keep = false;
    if (j < 0) keep = (long long)cnt >= min_chain_length;
    else if (f0 - (long long)s.f((uint32_t)j - fb) >= min_chain_score) keep = (long long)cnt >= min_chain_length;
    return cnt;
}

// chain.hpp:380-400 for one run: its ns chain starts, as cc_run_starts' emit put them into the start column (S::start(q) / S::set_start(q, v): global anchor
// indices below 255), are taken in cc_start_before's order - the next one is looked for among those not yet done, which are then marked 255 - and backtracked.
// visit(j) gets a chain's anchors right to left, then chain(j0, f0, cnt, keep) the chain: its start, score, number of anchors and whether it is kept.
template <class S, class Visit, class Chain>
CC_HD void cc_run_chains(S& s, uint32_t fb, uint32_t n, uint32_t ns, long long min_chain_score, long long min_chain_length, Visit visit, Chain chain) {
    for (uint32_t k = 0; k < n; ++k) s.set_t(k, 0);
    for (uint32_t it = 0; it < ns; ++it) {
        uint32_t best = 0xFFu, bj = 0; int32_t bf = 0;
        for (uint32_t q = 0; q < ns; ++q) {
            const uint32_t j = (uint32_t)s.start(q);
            if (j == 0xFFu) continue;
            const int32_t fj = (int32_t)s.f(j - fb);
            if (best == 0xFFu || cc_start_before(fj, j, bf, bj)) { best = q; bj = j; bf = fj; }
        }
        s.set_start(best, 0xFF);
        bool keep;
        const uint32_t cnt = cc_run_backtrack(s, fb, bj, min_chain_score, min_chain_length, keep, visit);
        chain(bj, bf, cnt, keep);
    }
}

// The place of kept chain c of a read among its n kept chains in the order the sorted starts append them (chain.hpp:380-400): by (score, start index)
// descending.  key[s] = score << 8 | start index of chain s, the chains listed run by run and inside a run in the order they were backtracked; equal pairs
// are two ends of one run that gave the same start, and stay in the order they were walked.  The chains then go through std::sort by score alone
// (chain.hpp:402): up to 16 of them that is one insertion sort, a stable sort, which keeps this order; more go through the introsort (sort_emul.h).
CC_HD uint32_t cc_chain_pos(const uint32_t* key, uint32_t n, uint32_t c) {
    const uint32_t kc = key[c];
    uint32_t pos = 0;
#pragma unroll 8
    for (uint32_t s = 0; s < n; ++s) pos += (key[s] > kc || (key[s] == kc && s < c)) ? 1u : 0u;
    return pos;
}
