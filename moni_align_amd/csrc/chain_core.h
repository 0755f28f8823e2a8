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
