// The run-level chaining routines of chain_core.h (cc_run_dp, cc_run_starts, cc_start_before, cc_run_chains, cc_run_backtrack, cc_chain_pos) through a column
// accessor of the widths chain_runs_kernel uses (16-bit f / msc, 8-bit p / t holding global anchor indices), against the whole-read serial form
// (ac_chain, align_core.h).  A program of its own: g++ -std=c++17 [-fsanitize=address,undefined] chain_runs_sim.cpp; usage: chain_runs_sim [seed].
//   check 1  f / p / msc of every anchor, the kept chains, their order and their anchor lists equal the serial form's;
//   check 2  a run chained as the read's first run and behind a copy of itself gives the same chains (p > 0 and t == i compare global indices);
//   guard words on both sides of every column, and the columns of the lanes without a run, must come back untouched.
// Prints histograms (starts of a run, dropped chains, kept chains of a read) and "OK <reads> <runs> <chains>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <algorithm>

#include "../../moni_align_amd/csrc/align_core.h"

static const int RUN_LEN = 8, SLOTS = 16, MAX_NA = 96, MAX_CH = 48;
static const uint32_t GUARD = 0xA5C3u;

struct rng_t {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    uint32_t below(uint32_t n) { return next() % n; }
};

// one lane's columns, a guard word on both sides of each
struct col_t {
    uint64_t node[RUN_LEN + 2]; int16_t f[RUN_LEN + 2], msc[RUN_LEN + 2]; int8_t p[RUN_LEN + 2]; uint8_t t[RUN_LEN + 2], sj[RUN_LEN + 2];
    void init() {
        for (int k = 0; k < RUN_LEN + 2; ++k) { node[k] = 0x5A5A5A5A5A5A5A5Aull; f[k] = msc[k] = (int16_t)GUARD; p[k] = (int8_t)0x5A; t[k] = sj[k] = 0xA5; }
    }
    bool guards_ok() const {
        for (int k : {0, RUN_LEN + 1}) if (node[k] != 0x5A5A5A5A5A5A5A5Aull || f[k] != (int16_t)GUARD || msc[k] != (int16_t)GUARD || p[k] != (int8_t)0x5A || t[k] != 0xA5 || sj[k] != 0xA5) return false;
        return true;
    }
    bool untouched() const {
        for (int k = 0; k < RUN_LEN + 2; ++k) if (node[k] != 0x5A5A5A5A5A5A5A5Aull || f[k] != (int16_t)GUARD || msc[k] != (int16_t)GUARD || p[k] != (int8_t)0x5A || t[k] != 0xA5 || sj[k] != 0xA5) return false;
        return true;
    }
};
struct acc_t {          // the accessor of chain_core.h over one lane's columns; node: x - xbase | rpos << 32 | len << 42 | idx << 52 | mate << 62
    col_t& c;
    long long x(uint32_t k) const { return (long long)(uint32_t)c.node[k + 1]; }
    int32_t y(uint32_t k) const { return (int32_t)((c.node[k + 1] >> 32) & 1023u); }
    int32_t w(uint32_t k) const { return (int32_t)((c.node[k + 1] >> 42) & 1023u); }
    uint32_t mate(uint32_t k) const { return (uint32_t)(c.node[k + 1] >> 62); }
    int32_t f(uint32_t k) const { return c.f[k + 1]; }
    int32_t msc(uint32_t k) const { return c.msc[k + 1]; }
    int32_t p(uint32_t k) const { return c.p[k + 1]; }
    int32_t t(uint32_t k) const { return c.t[k + 1]; }
    void set_f(uint32_t k, int32_t v) { c.f[k + 1] = (int16_t)v; }
    void set_msc(uint32_t k, int32_t v) { c.msc[k + 1] = (int16_t)v; }
    void set_p(uint32_t k, int32_t v) { c.p[k + 1] = (int8_t)v; }
    void set_t(uint32_t k, int32_t v) { c.t[k + 1] = (uint8_t)v; }
    uint32_t start(uint32_t q) const { return c.sj[q + 1]; }
    void set_start(uint32_t q, uint32_t v) { c.sj[q + 1] = (uint8_t)v; }
};

struct seed_t { uint32_t idx, len, strand; };
struct chain_out_t { int32_t score; std::vector<uint32_t> an; };          // anchors right to left, global indices

// a read: seeds and, run by run, which seeds occur there and at which text position; returns false if the read has more than MAX_NA anchors
struct read_t {
    std::vector<seed_t> seeds;
    std::vector<std::vector<uint64_t>> occs;          // per seed
};

static ac_params_t params(long long max_pred, long long max_iter, long long min_score) {
    ac_params_t P; memset(&P, 0, sizeof P);
    P.max_dist_x = 500; P.max_dist_y = 100; P.max_iter = max_iter; P.max_pred = max_pred; P.min_chain_score = min_score; P.min_chain_length = 1;
    return P;
}

// the serial form over the read; fills the sorted anchors' nodes (W.anch / W.node) and the chains
static bool serial(ac_ws_t& W, const ac_params_t& P, const read_t& R) {
    ac_reset(W);
    for (size_t s = 0; s < R.seeds.size(); ++s) {
        if (R.occs[s].empty()) continue;
        ac_mem_t& M = W.mems[W.n_mems++];
        M.pos = R.occs[s][0]; M.len = R.seeds[s].len; M.idx = R.seeds[s].idx; M.rpos = R.seeds[s].idx + R.seeds[s].len - 1; M.mate = R.seeds[s].strand ? 2u : 0u;
        M.occs = R.occs[s].data(); M.nocc = (uint32_t)R.occs[s].size();
    }
    return ac_chain(W, P);
}

// the runs of the sorted anchors by the column routines; out: the kept chains in their final order (cc_chain_pos, then std::sort by score: the introsort
// emulation, which is an insertion sort up to 16), or false when there are more than MAX_CH (the kernel hands such a read to the large instance).  per_run (optional): the chains of every run in backtracking order, kept or not
static bool by_runs(const ac_ws_t& W, const ac_params_t& P, float avg, std::vector<chain_out_t>& out, std::vector<int32_t>& F, std::vector<int32_t>& PP, std::vector<int32_t>& MSC,
                    unsigned long* h_starts, unsigned long* n_dropped, std::vector<std::vector<chain_out_t>>* per_run, bool& guards) {
    const uint32_t na = W.n_anch;
    std::vector<uint32_t> rs;
    for (uint32_t i = 0; i < na; ++i) if (i == 0 || (long long)W.anch[i].x > (long long)W.anch[i - 1].x + P.max_dist_x) rs.push_back(i);
    rs.push_back(na);
    const uint32_t n_runs = (uint32_t)rs.size() - 1;
    if (n_runs > (uint32_t)SLOTS) { fprintf(stderr, "generator: %u runs\n", n_runs); exit(2); }
    static col_t cols[SLOTS];
    for (int l = 0; l < SLOTS; ++l) cols[l].init();
    uint32_t key[SLOTS * RUN_LEN];
    std::vector<chain_out_t> kept;          // run by run, in backtracking order
    F.assign(na, 0); PP.assign(na, 0); MSC.assign(na, 0);
    if (per_run) per_run->assign(n_runs, {});
    for (uint32_t r = 0; r < n_runs; ++r) {
        const uint32_t fb = rs[r], n = rs[r + 1] - fb;
        if (n > (uint32_t)RUN_LEN) { fprintf(stderr, "generator: run of %u\n", n); exit(2); }
        acc_t S{cols[r]};
        const uint64_t xbase = W.anch[fb].x;
        for (uint32_t k = 0; k < n; ++k) {
            const ac_mem_t& m = W.mems[W.anch[fb + k].mem];
            cols[r].node[k + 1] = (W.anch[fb + k].x - xbase) | ((uint64_t)m.rpos << 32) | ((uint64_t)m.len << 42) | ((uint64_t)m.idx << 52) | ((uint64_t)m.mate << 62);
            cols[r].t[k + 1] = 0;
        }
        cc_run_dp<int32_t, uint32_t>(S, fb, n, (int32_t)P.max_iter, (uint32_t)P.max_pred, P.max_dist_x, (int32_t)P.max_dist_y, avg);
        for (uint32_t k = 0; k < n; ++k) { F[fb + k] = S.f(k); PP[fb + k] = S.p(k); MSC[fb + k] = S.msc(k); }
        uint32_t ns = 0;
        cc_run_starts(S, fb, n, P.min_chain_score, [&](uint32_t j) { S.set_start(ns++, j); });
        if (h_starts) h_starts[ns < 8 ? ns : 7]++;
        chain_out_t c;
        bool bad = false;
        cc_run_chains(S, fb, n, ns, P.min_chain_score, P.min_chain_length, [&](uint32_t j) { c.an.push_back(j); },
                      [&](uint32_t j0, int32_t f0, uint32_t cnt, bool keep) {
            c.score = f0;
            bad = bad || cnt != c.an.size() || c.an[0] != j0;
            if (per_run) { chain_out_t d = c; if (!keep) d.score = -d.score - 1; for (auto& a : d.an) a -= fb; (*per_run)[r].push_back(d); }
            if (!keep) { if (n_dropped) ++*n_dropped; }
            else { key[kept.size()] = ((uint32_t)f0 << 8) | j0; kept.push_back(c); }
            c.an.clear();
        });
        if (bad) return false;
        for (uint32_t q = 0; q < ns; ++q) cols[r].sj[1 + q] = 0xA5;          // (so that `untouched` below means the lanes without a run)
    }
    guards = true;
    for (uint32_t l = 0; l < (uint32_t)SLOTS; ++l) guards = guards && (l < n_runs ? cols[l].guards_ok() : cols[l].untouched());
    out.clear();
    if (kept.size() > (size_t)MAX_CH) return false;
    const uint32_t nk = (uint32_t)kept.size();
    std::vector<uint32_t> ord(nk), seen(nk, 0);
    for (uint32_t c = 0; c < nk; ++c) { const uint32_t pos = cc_chain_pos(key, nk, c); if (pos >= nk || seen[pos]++) { guards = false; return true; } ord[pos] = (key[c] & ~0xFFu) | c; }
    lsort::sort(ord.data(), (long)nk, [](const uint32_t& x, const uint32_t& y) { return (x >> 8) > (y >> 8); });
    for (uint32_t k = 0; k < nk; ++k) out.push_back(kept[ord[k] & 0xFFu]);
    return true;
}

// seeds of a read (the halves of a MEM end where it ends: tied reference ends) and runs that hold subsets of them
static read_t make_read(rng_t& g, uint32_t n_runs, uint32_t max_len, bool equal_runs, bool mix_strands) {
    read_t R;
    const uint32_t n_seeds = 3 + g.below(14);
    for (uint32_t s = 0; s < n_seeds; ++s) {
        seed_t sd; sd.idx = g.below(120); sd.len = 25 + g.below(40); sd.strand = mix_strands ? g.below(2) : 0;
        if (s > 0 && g.below(4) == 0) { const seed_t& o = R.seeds[g.below(s)]; sd.len = o.len > 30 ? o.len / 2 : o.len; sd.idx = o.idx + o.len - sd.len; sd.strand = o.strand; }      // a right half: same end
        R.seeds.push_back(sd);
    }
    R.occs.assign(n_seeds, {});
    uint32_t na = 0;
    std::vector<uint32_t> pick0; std::vector<int> jit0;
    for (uint32_t r = 0; r < n_runs; ++r) {
        const uint64_t base = 100000ull + (uint64_t)r * 50000ull + (equal_runs ? 0 : g.below(1000));
        uint32_t len = 1 + g.below(max_len);
        if (na + len > (uint32_t)MAX_NA) len = MAX_NA - na;
        if (len == 0) break;
        std::vector<uint32_t> pick; std::vector<int> jit;
        if (equal_runs && r > 0) { if (na + pick0.size() > (size_t)MAX_NA) break; pick = pick0; jit = jit0; }
        else for (uint32_t k = 0; k < len; ++k) { pick.push_back(g.below(n_seeds)); jit.push_back(g.below(3) == 0 ? (int)g.below(40) - 20 : 0); }
        if (r == 0) { pick0 = pick; jit0 = jit; }
        for (size_t k = 0; k < pick.size(); ++k) R.occs[pick[k]].push_back(base + R.seeds[pick[k]].idx + (uint64_t)(100 + jit[k]));
        na += (uint32_t)pick.size();
    }
    return R;
}

int main(int argc, char** argv) {
    rng_t g{argc > 1 ? strtoull(argv[1], nullptr, 10) : 1ull};
    ac_ws_t* W = new ac_ws_t();
    ac_ws_t* W2 = new ac_ws_t();
    unsigned long reads = 0, runs = 0, chains = 0, dropped = 0, many = 0, first_checked = 0, h_starts[8] = {}, h_kept[MAX_CH + 2] = {}, tied = 0;
    for (long long max_pred : {1ll, 5ll}) for (long long max_iter : {2ll, 10ll}) for (long long min_score : {0ll, 20ll, 40ll}) {
        const ac_params_t P = params(max_pred, max_iter, min_score);
        for (int trial = 0; trial < 1500; ++trial) {
            const uint32_t n_runs = trial % 50 == 0 ? 16 : 1 + g.below(16), max_len = trial % 7 == 0 ? RUN_LEN : 1 + g.below(RUN_LEN);
            const read_t R = make_read(g, n_runs, max_len, trial % 5 == 1, trial % 3 == 0);
            const bool chained = serial(*W, P, R);
            if (W->overflow) { fprintf(stderr, "generator: the serial form overflowed\n"); return 2; }
            if (W->n_anch == 0) continue;
            size_t tot_len = 0;
            for (uint32_t i = 0; i < W->n_mems; ++i) tot_len += (size_t)W->mems[i].len * W->mems[i].nocc;
            const float avg = (float)tot_len / (size_t)W->n_anch;
            std::vector<chain_out_t> out; std::vector<int32_t> F, PP, MSC; bool guards = false;
            std::vector<std::vector<chain_out_t>> per_run;
            const bool ordered = by_runs(*W, P, avg, out, F, PP, MSC, h_starts, &dropped, &per_run, guards);
            if (!guards) { printf("FAIL guard words or the places of the chains, trial %d\n", trial); return 1; }
            ++reads; runs += per_run.size();
            // check 1: the DP
            for (uint32_t i = 0; i < W->n_anch; ++i) {
                if (F[i] != W->node[i].f || PP[i] != W->node[i].p || MSC[i] != W->node[i].msc) {
                    printf("FAIL DP: trial %d anchor %u f %d/%d p %d/%d msc %d/%d\n", trial, i, F[i], W->node[i].f, PP[i], W->node[i].p, MSC[i], W->node[i].msc); return 1;
                }
                if (i > 0 && W->anch[i].x == W->anch[i - 1].x) ++tied;
            }
            // ... and the chains
            if (!ordered) { ++many; continue; }
            h_kept[out.size()]++;
            if (!chained) { if (!out.empty() && W->n_chains != 0) { printf("FAIL: trial %d chains where the serial form has none\n", trial); return 1; } if (out.empty()) continue; }
            if (out.size() != W->n_chains) { printf("FAIL: trial %d %zu chains, serial %u\n", trial, out.size(), W->n_chains); return 1; }
            for (uint32_t c = 0; c < W->n_chains; ++c) {
                const ac_chain_t& ch = W->chains[c];
                bool same = ch.score == out[c].score && ch.cnt == out[c].an.size();
                for (uint32_t k = 0; same && k < ch.cnt; ++k) same = W->pool[ch.off + k] == out[c].an[k];
                if (!same) { printf("FAIL: trial %d chain %u differs from the serial form's (score %lld / %d, %u / %zu anchors)\n", trial, c, ch.score, out[c].score, ch.cnt, out[c].an.size()); return 1; }
            }
            chains += out.size();
            // check 2: every run of the read alone in a read, and behind a copy of itself 50 000 bases to the left (the same seeds: the same average)
            if (trial % 4 == 0) for (size_t r = 0; r < per_run.size() && r < 3; ++r) {
                uint64_t lo = ~0ull, hi = 0;
                std::vector<uint32_t> rsv;
                for (uint32_t i = 0; i < W->n_anch; ++i) if (i == 0 || (long long)W->anch[i].x > (long long)W->anch[i - 1].x + P.max_dist_x) rsv.push_back(i);
                rsv.push_back(W->n_anch);
                lo = W->anch[rsv[r]].x; hi = W->anch[rsv[r + 1] - 1].x;
                bool ties = false;          // (the order of tied anchors is the introsort's and depends on the read's size: such a run is no longer the same run)
                for (uint32_t i = rsv[r] + 1; i < rsv[r + 1]; ++i) ties = ties || W->anch[i].x == W->anch[i - 1].x;
                if (ties) continue;
                read_t A, B; A.seeds = B.seeds = R.seeds; A.occs.assign(R.seeds.size(), {}); B.occs.assign(R.seeds.size(), {});
                for (size_t s = 0; s < R.seeds.size(); ++s) for (uint64_t o : R.occs[s]) {
                    const uint64_t x = o + R.seeds[s].len - 1;
                    if (x < lo || x > hi) continue;
                    A.occs[s].push_back(o); B.occs[s].push_back(o - 50000); B.occs[s].push_back(o);
                }
                std::vector<std::vector<chain_out_t>> pa, pb; std::vector<chain_out_t> oa, ob; bool ga = false, gb = false;
                serial(*W2, P, A);
                size_t tl = 0; for (uint32_t i = 0; i < W2->n_mems; ++i) tl += (size_t)W2->mems[i].len * W2->mems[i].nocc;
                const float avg_a = (float)tl / (size_t)W2->n_anch;
                by_runs(*W2, P, avg_a, oa, F, PP, MSC, nullptr, nullptr, &pa, ga);
                serial(*W2, P, B);
                tl = 0; for (uint32_t i = 0; i < W2->n_mems; ++i) tl += (size_t)W2->mems[i].len * W2->mems[i].nocc;
                const float avg_b = (float)tl / (size_t)W2->n_anch;
                by_runs(*W2, P, avg_b, ob, F, PP, MSC, nullptr, nullptr, &pb, gb);
                if (!ga || !gb || avg_a != avg_b || pa.size() != 1 || pb.size() != 2) { printf("FAIL: trial %d, the run alone and twice: %zu and %zu runs\n", trial, pa.size(), pb.size()); return 1; }
                for (int which = 0; which < 2; ++which) {
                    const auto& x = pa[0]; const auto& y = pb[which];
                    bool same = x.size() == y.size();
                    for (size_t c = 0; same && c < x.size(); ++c) same = x[c].score == y[c].score && x[c].an == y[c].an;
                    if (!same) { printf("FAIL: trial %d run %zu gives other chains as run %d of a read than as its first\n", trial, r, which); return 1; }
                }
                ++first_checked;
            }
        }
    }
    printf("starts of a run 0..7+:"); for (int k = 0; k < 8; ++k) printf(" %d:%lu", k, h_starts[k]); printf("\n");
    printf("kept chains of a read:"); for (int k = 0; k <= MAX_CH; ++k) printf(" %d:%lu", k, h_kept[k]); printf("\n");
    printf("dropped %lu tied_x %lu more_than_%d %lu first_and_not_first %lu\n", dropped, tied, MAX_CH, many, first_checked);
    printf("OK %lu %lu %lu\n", reads, runs, chains);
    delete W; delete W2;
    return 0;
}
