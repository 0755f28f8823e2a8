// TEST HARNESS ONLY - not part of the product, never linked into libmoni_hip.so.
// A program of its own (tests/test_host_ms_leap.py builds it plain and with the address and undefined-behaviour sanitizers) over the host copy of the
// index image, with the batch laid out as moni_reads_upload and pack_kernel lay it out, for the leaping walk of moni_align_amd/csrc/seed_core.h:
//  * the relation the leap rests on: with a suffix array of the text made here by prefix doubling, the BWT position of the walk is ISA[sample] in the
//    start state and after every step of every task, except behind an absent byte until the next jump (counted), and except where a decrement of
//    sample 0 has wrapped (counted; a walk in that state asks for no comparison);
//  * the tables (isa_walk_run, leap_clean_chunk) at strides 8, 16 and 32: every entry is the settled (run, off) of ISA[t], every clean byte the count
//    of A / C / G / T bytes from t on; no word outside the tables is written;
//  * ms_task_events_leap against ms_task_events<1, true> at the three strides, all tasks and over a live list: the event buffers (guards and unowned
//    words included), the counts, steps and jumps are identical.
// It prints the lengths of the matched stretches behind a jump that the batch holds, how many leapable stretches end on a multiple of the stride, and
// the leap statistics; the leaps of every task at the default stride go to the output file (u32 each).
//
// in:  as ms_events_sim's
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "../../moni_align_amd/csrc/image.hpp"
#include "../../moni_align_amd/csrc/seed_core.h"

template <class Tp>
static bool rd(FILE* f, std::vector<Tp>& v, size_t n) { v.resize(n); return !n || fread(v.data(), sizeof(Tp), n, f) == n; }

static const uint64_t GUARD = 0x5EED5EED5EED5EEDull;
static const uint32_t GUARD32 = 0x5EED5EEDu;
static const size_t PAD = 8;

#define FAIL(...) do { printf("FAIL: " __VA_ARGS__); printf("\n"); return 1; } while (0)

// suffix array of s[0 .. n) (s[n - 1] is the unique smallest byte) by prefix doubling
static std::vector<uint64_t> suffix_array(const std::vector<uint8_t>& s) {
    const size_t n = s.size();
    std::vector<uint64_t> sa(n), rk(n), tmp(n);
    for (size_t i = 0; i < n; ++i) { sa[i] = i; rk[i] = s[i]; }
    for (size_t k = 1;; k <<= 1) {
        auto key = [&](uint64_t i) { return std::make_pair(rk[i], i + k < n ? rk[i + k] + 1 : (uint64_t)0); };
        std::sort(sa.begin(), sa.end(), [&](uint64_t a, uint64_t b) { return key(a) < key(b); });
        tmp[sa[0]] = 0;
        for (size_t i = 1; i < n; ++i) tmp[sa[i]] = tmp[sa[i - 1]] + (key(sa[i - 1]) < key(sa[i]) ? 1 : 0);
        rk = tmp;
        if (rk[sa[n - 1]] == n - 1) break;
    }
    return sa;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint64_t> h, F, starts, ssa, esa, thr, slcp, seq_starts, offs;
    std::vector<uint8_t> heads, seq, text;
    bool ok = rd(f, h, 8);
    if (ok) {
        const uint64_t r = h[1];
        ok = rd(f, F, 256) && rd(f, starts, r + 1) && rd(f, ssa, r) && rd(f, esa, r) && rd(f, thr, r) && (!h[4] || rd(f, slcp, r)) && rd(f, seq_starts, h[3] + 1) &&
             rd(f, offs, h[5] + 1) && rd(f, heads, r) && rd(f, seq, offs.empty() ? 0 : offs.back()) && rd(f, text, h[0] - 1);
    }
    fclose(f);
    if (!ok) { fprintf(stderr, "ms_leap_sim: short input\n"); return 2; }
    moni_flat_index_t fi;
    memset(&fi, 0, sizeof fi);
    fi.n = h[0]; fi.r = h[1]; fi.w = h[2]; fi.n_seq = h[3];
    fi.F = F.data(); fi.heads = heads.data(); fi.starts = starts.data(); fi.ssa = ssa.data(); fi.esa = esa.data(); fi.thr = thr.data();
    fi.slcp = h[4] ? slcp.data() : nullptr; fi.seq_starts = seq_starts.data();
    HostImage img;
    if (img.build(fi)) { fprintf(stderr, "ms_leap_sim: %s\n", img.err.c_str()); return 3; }
    lds_tables_t L;
    memcpy(L.code, img.T.code, 256);
    memcpy(L.compl_tab, img.T.compl_tab, 256);
    for (int i = 0; i < 256; ++i) L.c2[i] = base_acgt((uint32_t)i) ? (uint8_t)base2((uint32_t)i) : (uint8_t)4;
    memcpy(L.abs_run, img.T.abs_run, sizeof(L.abs_run));
    memcpy(L.abs_pos, img.T.abs_pos, sizeof(L.abs_pos));
    for (int i = 0; i < MONI_MAX_SIGMA; ++i) { L.rec_base[i] = img.K.rec_base[i]; L.rec_cnt[i] = img.K.rec_cnt[i]; L.hot_slot[i] = img.K.hot_slot[i]; }
    const moni_consts_t& K = img.K;
    const uint64_t n = K.n, r = K.r, n_text = K.n_text;
    const moni_row_t* rows = img.rows.data(); const moni_frow_t* frows = img.frows.data(); const uint32_t* cr = img.cr.data(); const moni_rec_t* recs = img.recs.data();

    // ---- the suffix array and its inverse ---------------------------------------------------------------------------------------------------------
    std::vector<uint64_t> isa_full(n);
    {
        std::vector<uint8_t> s(text);
        for (uint8_t b : s) if (b < 2) FAIL("the text holds a byte below 2");
        s.push_back(0);
        const std::vector<uint64_t> sa = suffix_array(s);
        for (uint64_t i = 0; i < n; ++i) isa_full[sa[i]] = i;
        for (uint64_t k = 0; k < r; ++k) if ((sa[starts[k]] + n - 1) % n != ssa[k]) FAIL("run %llu: ssa is not SA[start] - 1", (unsigned long long)k);
        if (sa[n - 1] != K.last_run_sample) FAIL("last_run_sample is not SA[n - 1]");
    }

    // ---- the batch ----------------------------------------------------------------------------------------------------------------------------------
    const uint64_t n_reads = h[5], n_tasks = 2 * n_reads;
    const uint64_t n_blk = (n_reads + 31) / 32;
    std::vector<moni_u64x2> blk(n_blk + 1);
    {
        uint64_t pw = 0, qw = 0;
        for (uint64_t k = 0; k < n_blk; ++k) {
            uint64_t lb = 0;
            for (uint64_t i = 32 * k; i < n_reads && i < 32 * k + 32; ++i) lb = std::max<uint64_t>(lb, offs[i + 1] - offs[i]);
            blk[k].x = qw; blk[k].y = pw;
            qw += 64 * lb; pw += 64 * ws_pat_words(lb);
        }
        blk[n_blk].x = qw; blk[n_blk].y = pw;
    }
    std::vector<uint64_t> pat(blk[n_blk].y);
    std::vector<uint8_t> pflag(n_tasks, 0xEE);
    std::vector<uint64_t> seq_pad((offs[n_reads] + 16 + 7) / 8 + 1, 0);
    if (offs[n_reads]) memcpy(seq_pad.data(), seq.data(), offs[n_reads]);
    const uint8_t* sq = reinterpret_cast<const uint8_t*>(seq_pad.data());
    for (uint64_t t = 0; t < n_tasks; ++t) pack_task(L, sq, offs.data(), blk.data(), t, pat.data(), pflag.data());
    auto len_of = [&](uint64_t t) { return (uint32_t)(offs[(t >> 1) + 1] - offs[t >> 1]); };

    // ---- the relation: position == ISA[sample], step by step (the loop of ms_task) ------------------------------------------------------------------
    unsigned long long n_checked = 0, n_behind_absent = 0, n_wrapped = 0;
    std::set<uint32_t> stretch_lens;
    unsigned long long on_multiple[3] = {0, 0, 0}, leapable[3] = {0, 0, 0};
    auto position = [&](const ms_state_t& S) -> uint64_t {
        if (S.abs) return S.pos;
        if (S.off == MONI_OFF_END) return ld_start(rows, S.run + 1) - 1;
        return row_start(rows[S.run]) + S.off;
    };
    for (uint64_t t = 0; t < n_tasks; ++t) {
        const uint32_t m = len_of(t);
        const uint64_t pb = ws_pat_base(blk.data(), t);
        ms_state_t S;
        S.m = m; S.run = (uint32_t)r - 1; S.pos = n - 1; S.abs = true; S.off = 0; S.sample = K.last_run_sample; S.word = 0;
        if (position(S) != isa_full[S.sample]) FAIL("the start state is not ISA[last_run_sample]");
        bool valid = true;
        uint32_t cnt = 0; uint64_t at_jump = S.sample;
        auto close = [&]() {          // a stretch of cnt matches behind a jump (or the start) that assigned at_jump
            if (!valid) return;
            stretch_lens.insert(cnt);
            for (uint32_t x = 0; x < 3; ++x) {
                const uint32_t stride = 8u << x;
                if (cnt >= MONI_LEAP_T + stride + MONI_LEAP_KMIN && at_jump >= cnt) { ++leapable[x]; if (!((at_jump - cnt) & (stride - 1))) ++on_multiple[x]; }
            }
        };
        unsigned long long nj = 0;
        for (uint32_t s = 0; s < m; ++s) {
            const uint32_t raw = (uint32_t)(pat[pb + (uint64_t)(s >> 3) * 64u] >> (8 * (s & 7))) & 0xFFu;
            const uint32_t c = L.code[raw];
            if (c == MONI_CODE_ABSENT) { close(); S.sample = 0; S.pos = L.abs_pos[raw]; S.run = L.abs_run[raw]; S.abs = true; valid = false; cnt = 0; ++n_behind_absent; continue; }
            const unsigned long long j0 = nj;
            const uint64_t before = S.sample;
            ms_step(K, L, rows, frows, cr, recs, c, S, nj);
            if (nj != j0) { close(); valid = true; cnt = 0; at_jump = S.sample; }
            else {
                ++cnt;
                if (valid && before >= 1 && before <= n_text && base_acgt(raw) && text[before - 1] != raw) FAIL("task %llu step %u: a matched step whose byte is not text[sample - 1]", (unsigned long long)t, s);
            }
            if (!valid) { ++n_behind_absent; continue; }
            if (S.sample >= n) { ++n_wrapped; continue; }
            if (position(S) != isa_full[S.sample]) FAIL("task %llu step %u: position %llu, ISA[%llu] = %llu", (unsigned long long)t, s, (unsigned long long)position(S), (unsigned long long)S.sample, (unsigned long long)isa_full[S.sample]);
            ++n_checked;
        }
        close();
    }

    // ---- the tables ---------------------------------------------------------------------------------------------------------------------------------
    std::vector<uint8_t> text_pad(n_text + 16, 0);
    memcpy(text_pad.data(), text.data(), n_text);
    std::vector<uint64_t> text2(n_text / 32 + 2, 0);
    for (uint64_t w = 0; w < text2.size(); ++w) { bool bad; text2[w] = text2_word(text_pad.data(), n_text, w, bad); }
    std::vector<uint64_t> isa_t[3], clean_t[3];
    for (uint32_t x = 0; x < 3; ++x) {
        const uint32_t sh = 3 + x;
        const uint64_t n_ent = ((n - 1) >> sh) + 1, clean_words = n_ent / 8 + 2;
        std::vector<uint64_t>& isa = isa_t[x]; std::vector<uint64_t>& cw = clean_t[x];
        isa.assign(PAD + n_ent + 2 + PAD, GUARD); cw.assign(PAD + clean_words + PAD, GUARD);
        std::fill(isa.begin() + PAD, isa.begin() + PAD + n_ent + 2, ~0ull);
        std::fill(cw.begin() + PAD, cw.begin() + PAD + clean_words, 0);
        uint8_t* clean = reinterpret_cast<uint8_t*>(cw.data() + PAD);
        for (uint64_t c0 = 0; c0 < n; c0 += 4096) leap_clean_chunk(text.data(), n_text, c0, std::min<uint64_t>(c0 + 4096, n), sh, clean);
        for (uint64_t k = 0; k < r; ++k) isa_walk_run(rows, r, n, k, ssa[k], sh, isa.data() + PAD, clean);
        for (size_t i = 0; i < PAD; ++i) if (isa[i] != GUARD || isa[isa.size() - 1 - i] != GUARD || cw[i] != GUARD || cw[cw.size() - 1 - i] != GUARD) FAIL("stride %u: a guard word of the tables was written", 1u << sh);
        if (isa[PAD + n_ent] != ~0ull || isa[PAD + n_ent + 1] != ~0ull) FAIL("stride %u: an entry behind the table was written", 1u << sh);
        for (uint64_t i = 0; i < n_ent; ++i) {
            const uint64_t t = i << sh, e = isa[PAD + i];
            if (e == ~0ull) FAIL("stride %u: entry %llu was not written", 1u << sh, (unsigned long long)i);
            const uint64_t run = e & 0xFFFFFFFFull, off = e >> 32;
            if (run >= r || starts[run] + off >= starts[run + 1]) FAIL("stride %u: entry %llu is not settled in its run", 1u << sh, (unsigned long long)i);
            if (starts[run] + off != isa_full[t]) FAIL("stride %u: entry %llu is position %llu, ISA[%llu] = %llu", 1u << sh, (unsigned long long)i, (unsigned long long)(starts[run] + off), (unsigned long long)t, (unsigned long long)isa_full[t]);
            uint32_t want = 0;
            while (want < MONI_LEAP_MAX && t + want < n_text && base_acgt(text[t + want])) ++want;
            if (clean[i] != want) FAIL("stride %u: clean byte %llu is %u, want %u", 1u << sh, (unsigned long long)i, clean[i], want);
        }
    }

    // ---- the walks ----------------------------------------------------------------------------------------------------------------------------------
    std::vector<uint64_t> live;
    std::vector<uint8_t> listed(n_tasks, 0);
    for (uint64_t rd_ = 0; rd_ < n_reads; ++rd_) {
        const uint64_t kind = (rd_ * 7 + 3) % 5;
        if (kind == 0) { listed[2 * rd_] = listed[2 * rd_ + 1] = 1; }
        else if (kind < 4) listed[2 * rd_ + ((rd_ + kind) & 1u)] = 1;
    }
    for (uint64_t t = 0; t < n_tasks; ++t) if (listed[t]) live.push_back(t);
    const uint64_t n_live = live.size();
    live.push_back(~0ull);
    const uint64_t ev_words = ws_ev_words(blk[n_blk].x, n_blk);
    struct EvRun { std::vector<uint64_t> ev; std::vector<uint32_t> cnt; std::vector<uint64_t> col; unsigned long long steps = 0, jumps = 0; };
    auto fresh = [&](EvRun& E) { E.ev.assign(PAD + ev_words + PAD, GUARD); E.cnt.assign(PAD + n_tasks + PAD, GUARD32); E.col.assign(1 + MONI_EV_STAGE_N + 1, GUARD); E.steps = E.jumps = 0; };
    EvRun R[2];                 // the stepwise walk: every task, the live list
    for (int v = 0; v < 2; ++v) {
        fresh(R[v]);
        const uint64_t nt = v ? n_live : n_tasks;
        for (uint64_t g = 0; g < nt; ++g)
            ms_task_events<1, true>(K, L, rows, frows, cr, recs, pat.data(), offs.data(), blk.data(), nt, g, R[v].ev.data() + PAD, R[v].cnt.data() + PAD, R[v].steps, R[v].jumps, v ? live.data() : nullptr, R[v].col.data() + 1, 1);
    }
    std::vector<uint32_t> task_leaps(n_tasks, 0);
    unsigned long long tot[3][3];
    for (uint32_t x = 0; x < 3; ++x) {
        ms_leap_t Z; Z.isa = isa_t[x].data() + PAD; Z.clean = clean_t[x].data() + PAD; Z.text2 = text2.data(); Z.n_text = n_text; Z.sh = 3 + x;
        for (int q = 0; q < 3; ++q) tot[x][q] = 0;
        for (int v = 0; v < 2; ++v) {
            EvRun E; fresh(E);
            const uint64_t nt = v ? n_live : n_tasks;
            for (uint64_t g = 0; g < nt; ++g) {
                unsigned long long st[3] = {0, 0, 0};
                ms_task_events_leap(K, L, rows, frows, cr, recs, pat.data(), offs.data(), blk.data(), nt, g, E.ev.data() + PAD, E.cnt.data() + PAD, E.steps, E.jumps, v ? live.data() : nullptr, E.col.data() + 1, 1, Z, pflag.data(), st);
                if (!v) { for (int q = 0; q < 3; ++q) tot[x][q] += st[q]; if (x == MONI_LEAP_SH - 3u) task_leaps[g] = (uint32_t)st[0]; }
                if (st[1] > len_of(v ? live[g] : g) || st[0] > st[2]) FAIL("stride %u, task %llu: %llu steps leapt in %llu leaps of %llu comparisons", 8u << x, (unsigned long long)g, st[1], st[0], st[2]);
            }
            if (E.col.front() != GUARD || E.col.back() != GUARD) FAIL("stride %u: a guard word of the stage was written", 8u << x);
            if (E.steps != R[v].steps || E.jumps != R[v].jumps) FAIL("stride %u%s: %llu steps, %llu jumps; stepwise %llu, %llu", 8u << x, v ? ", live list" : "", E.steps, E.jumps, R[v].steps, R[v].jumps);
            if (E.cnt != R[v].cnt) FAIL("stride %u%s: the event counts differ from the stepwise walk's", 8u << x, v ? ", live list" : "");
            if (E.ev != R[v].ev) {
                size_t i = 0; while (E.ev[i] == R[v].ev[i]) ++i;
                FAIL("stride %u%s: the event buffers differ at word %zu: %llx, stepwise %llx", 8u << x, v ? ", live list" : "", i - PAD, (unsigned long long)E.ev[i], (unsigned long long)R[v].ev[i]);
            }
        }
    }

    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    ok = !n_tasks || fwrite(task_leaps.data(), 4, n_tasks, o) == n_tasks;
    if (fclose(o) != 0 || !ok) return 2;
    printf("stretches:");
    for (uint32_t v : stretch_lens) printf(" %u", v);
    printf("\nleapable stretches (on a multiple of the stride): 8: %llu (%llu), 16: %llu (%llu), 32: %llu (%llu)\n", leapable[0], on_multiple[0], leapable[1], on_multiple[1], leapable[2], on_multiple[2]);
    printf("leaps / steps leapt / comparisons: 8: %llu %llu %llu, 16: %llu %llu %llu, 32: %llu %llu %llu\n", tot[0][0], tot[0][1], tot[0][2], tot[1][0], tot[1][1], tot[1][2], tot[2][0], tot[2][1], tot[2][2]);
    printf("OK: %llu reads, %llu steps, %llu jumps, %llu steps checked against the suffix array, %llu behind an absent byte, %llu wrapped\n",
           (unsigned long long)n_reads, R[0].steps, R[0].jumps, n_checked, n_behind_absent, n_wrapped);
    return 0;
}
