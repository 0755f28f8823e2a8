// chain_core.h: the narrow (32-bit) form of the chaining DP's per-predecessor arithmetic equals the wide (reference) form for every case that the
// predicate cc_narrow_ok admits, at the predicate's own bounds, and the predicate rejects parameters one beyond each bound.  Prints "OK <cases>".
#include <stdio.h>
#include <stdint.h>
#include <vector>
#include "../../moni_align_amd/csrc/chain_core.h"

struct params_t { long long max_dist_x, max_dist_y, max_iter, max_pred; };

static long long n_cases = 0, n_fail = 0;

static void one(long long x_d, long long y_i, long long y_j, long long w_i, bool same, long long max_dist_y, float avg) {
    long long gw = 0; int32_t gn = 0;
    const bool kw = cc_gain<long long>(x_d, y_i, y_j, w_i, same, max_dist_y, avg, gw);
    const bool kn = cc_gain<int32_t>((int32_t)x_d, (int32_t)y_i, (int32_t)y_j, (int32_t)w_i, same, (int32_t)max_dist_y, avg, gn);
    ++n_cases;
    if (kw != kn || (kw && gw != (long long)gn)) {
        if (n_fail++ < 10) printf("differs: x_d %lld y_i %lld y_j %lld w %lld same %d max_dist_y %lld avg %g: wide %d %lld narrow %d %d\n", x_d, y_i, y_j, w_i, (int)same, max_dist_y, avg, (int)kw, gw, (int)kn, gn);
    }
}

int main() {
    // ---- the predicate: its bounds pass, one beyond each fails ----
    const params_t dflt = {500, 100, 50, 50};
    int bad = 0;
    auto expect = [&](params_t p, bool want, const char* what) { if (cc_narrow_ok(p) != want) { printf("predicate: %s\n", what); ++bad; } };
    expect(dflt, true, "typical parameters");
    { params_t p = dflt; p.max_dist_x = CC_NARROW_MAX_DIST; expect(p, true, "max_dist_x at its bound"); p.max_dist_x += 1; expect(p, false, "max_dist_x above"); p.max_dist_x = 0; expect(p, true, "max_dist_x 0"); p.max_dist_x = -1; expect(p, false, "max_dist_x below"); }
    { params_t p = dflt; p.max_dist_y = CC_NARROW_MAX_DIST; expect(p, true, "max_dist_y at its bound"); p.max_dist_y += 1; expect(p, false, "max_dist_y above"); p.max_dist_y = -CC_NARROW_MAX_DIST; expect(p, true, "max_dist_y at its lower bound"); p.max_dist_y -= 1; expect(p, false, "max_dist_y below"); }
    { params_t p = dflt; p.max_iter = CC_NARROW_MAX_COUNT; expect(p, true, "max_iter at its bound"); p.max_iter += 1; expect(p, false, "max_iter above"); p.max_iter = 0; expect(p, true, "max_iter 0"); p.max_iter = -1; expect(p, false, "max_iter below"); }
    { params_t p = dflt; p.max_pred = CC_NARROW_MAX_COUNT; expect(p, true, "max_pred at its bound"); p.max_pred += 1; expect(p, false, "max_pred above"); p.max_pred = 0; expect(p, true, "max_pred 0"); p.max_pred = -1; expect(p, false, "max_pred below"); }

    // ---- narrow == wide ----
    // x_d: 0 and the values that put l = |y_d - x_d| at 0, 1, 2^k - 1, 2^k, 2^k + 1, up to the largest admitted distance
    std::vector<long long> xs = {0, 1, 2, 3};
    for (int k = 2; k <= 28; ++k) for (long long d = -1; d <= 1; ++d) { const long long v = (1ll << k) + d; if (v <= CC_NARROW_MAX_DIST) xs.push_back(v); }
    xs.push_back(CC_NARROW_MAX_DIST - 1); xs.push_back(CC_NARROW_MAX_DIST);
    // y_d: 0, +-1, +-(CC_MAX_READ - 1), and, for pairs whose second mate is placed behind the first, +-(2 * CC_MAX_READ - 1)
    const long long yd[] = {0, 1, -1, 2, -2, 7, -7, 100, -100, CC_MAX_READ - 1, -(CC_MAX_READ - 1), 2 * CC_MAX_READ - 1, -(2 * CC_MAX_READ - 1)};
    const float avgs[] = {25.f, 25.5f, 31.f, 33.333332f, 47.9f, 64.f, 99.99f, 100.f, 137.25f, 150.f, 255.875f, 300.1f, 511.f, 511.99f, 512.f};
    const long long ws[] = {1, 25, 150, CC_MAX_READ - 1};
    const long long mdys[] = {100, 0, -CC_NARROW_MAX_DIST, CC_NARROW_MAX_DIST, 2 * CC_MAX_READ};
    for (long long x0 : xs)
        for (long long y_d : yd) {
            // x_d itself, and the x_d that makes l = x0 for this y_d (l = |y_d - x_d|): x_d = y_d + x0 or y_d - x0 where that is a distance
            long long cand[3] = {x0, y_d + x0, y_d - x0};
            for (long long x_d : cand) {
                if (x_d < 0 || x_d > CC_NARROW_MAX_DIST) continue;
                for (float avg : avgs)
                    for (long long w : ws)
                        for (long long mdy : mdys)
                            for (int same = 0; same < 2; ++same) {
                                const long long y_j = y_d >= 0 ? 0 : -y_d, y_i = y_j + y_d;          // both in [0, 2 * CC_MAX_READ)
                                one(x_d, y_i, y_j, w, same != 0, mdy, avg);
                                const long long top = 2 * CC_MAX_READ - 1;
                                const long long y_j2 = y_d >= 0 ? top - y_d : top, y_i2 = y_j2 + y_d;
                                one(x_d, y_i2, y_j2, w, same != 0, mdy, avg);
                            }
            }
        }
    if (bad || n_fail) { printf("FAIL: %d predicate cases, %lld of %lld values differ\n", bad, n_fail, n_cases); return 1; }
    printf("OK %lld\n", n_cases);
    return 0;
}
