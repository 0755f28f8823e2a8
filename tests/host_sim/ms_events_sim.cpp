// TEST HARNESS ONLY - not part of the product, never linked into libmoni_hip.so.
// A program of its own (tests/test_host_ms_events.py builds it plain and with the address and undefined-behaviour sanitizers) over the host copy of
// the index image, with the batch laid out as moni_reads_upload and pack_kernel lay it out, for the event lists of moni_align_amd/csrc/seed_core.h:
//  * ms_task_events - a store per event with one and with two tasks per lane, staged eight at a time, and both over a live list - against ms_task:
//    the same steps and jumps, every variant the same lists, and every task's list expanded to the word of every step equals the dense pointer, word
//    for word (the wrapped decrement behind an absent byte included).  Lists are in step order, the first event covers step 0, nothing is written
//    outside a list: the event buffer, the counts and the stage stand between guard words, and every word that no list owns must stay a guard.
//  * mem_task from the dense source and from the event source, with and without the closed form over silent offsets, count pass and emit pass, at
//    two minimum lengths (the smaller one gives tasks with more than MONI_MEM_SLOTS MEMs, which the emit pass walks again): the same MEM records,
//    aux words, cnt_m, cnt_s, slots and n_cmp.
//
// in:  8 u64 (n, r, w, n_seq, has_lcp = 1, n_reads, 0, 0), F[256], starts[r + 1], ssa[r], esa[r], thr[r], slcp[r], seq_starts[n_seq + 1],
//      offs[n_reads + 1] (u64 each), then heads[r], the reads' bytes and the text's n - 1 bytes
// out: per read its pointers of strand 0, then those of strand 1 (the order of moni_ms_query_batch), then steps and jumps (u64 each)
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "../../moni_align_amd/csrc/image.hpp"
#include "../../moni_align_amd/csrc/seed_core.h"

template <class Tp>
static bool rd(FILE* f, std::vector<Tp>& v, size_t n) { v.resize(n); return !n || fread(v.data(), sizeof(Tp), n, f) == n; }

static const uint64_t GUARD = 0x5EED5EED5EED5EEDull;      // (no event: its step field is beyond every read here)
static const uint32_t GUARD32 = 0x5EED5EEDu;
static const size_t PAD = 8;

#define FAIL(...) do { printf("FAIL: " __VA_ARGS__); printf("\n"); return 1; } while (0)

struct EvRun {
    std::vector<uint64_t> ev; std::vector<uint32_t> cnt; std::vector<uint64_t> col;
    unsigned long long steps = 0, jumps = 0;
};

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
    if (!ok) { fprintf(stderr, "ms_events_sim: short input\n"); return 2; }
    moni_flat_index_t fi;
    memset(&fi, 0, sizeof fi);
    fi.n = h[0]; fi.r = h[1]; fi.w = h[2]; fi.n_seq = h[3];
    fi.F = F.data(); fi.heads = heads.data(); fi.starts = starts.data(); fi.ssa = ssa.data(); fi.esa = esa.data(); fi.thr = thr.data();
    fi.slcp = h[4] ? slcp.data() : nullptr; fi.seq_starts = seq_starts.data();
    HostImage img;
    if (img.build(fi)) { fprintf(stderr, "ms_events_sim: %s\n", img.err.c_str()); return 3; }
    lds_tables_t L;
    memcpy(L.code, img.T.code, 256);
    memcpy(L.compl_tab, img.T.compl_tab, 256);
    for (int i = 0; i < 256; ++i) L.c2[i] = base_acgt((uint32_t)i) ? (uint8_t)base2((uint32_t)i) : (uint8_t)4;
    memcpy(L.abs_run, img.T.abs_run, sizeof(L.abs_run));
    memcpy(L.abs_pos, img.T.abs_pos, sizeof(L.abs_pos));
    for (int i = 0; i < MONI_MAX_SIGMA; ++i) { L.rec_base[i] = img.K.rec_base[i]; L.rec_cnt[i] = img.K.rec_cnt[i]; L.hot_slot[i] = img.K.hot_slot[i]; }
    const moni_consts_t& K = img.K;

    const uint64_t n_reads = h[5], n_tasks = 2 * n_reads;
    // the workspace layout of reads_upload (moni_hip.hip): per block of 32 reads as many steps as its longest read has
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
    // exact sizes, so that a word read or written past the workspaces is the sanitizer's; pack_task reads aligned 8-byte words of a buffer padded by 16 bytes
    std::vector<uint64_t> pat(blk[n_blk].y);
    std::vector<uint64_t> seq_pad((offs[n_reads] + 16 + 7) / 8 + 1, 0);
    if (offs[n_reads]) memcpy(seq_pad.data(), seq.data(), offs[n_reads]);
    const uint8_t* sq = reinterpret_cast<const uint8_t*>(seq_pad.data());
    for (uint64_t t = 0; t < n_tasks; ++t) pack_task(L, sq, offs.data(), blk.data(), t, pat.data());
    auto len_of = [&](uint64_t t) { return (uint32_t)(offs[(t >> 1) + 1] - offs[t >> 1]); };

    const moni_row_t* rows = img.rows.data(); const moni_frow_t* frows = img.frows.data(); const uint32_t* cr = img.cr.data(); const moni_rec_t* recs = img.recs.data();
    // the dense pointers of every task
    std::vector<uint64_t> ptr(blk[n_blk].x, GUARD);
    unsigned long long d_steps = 0, d_jumps = 0;
    for (uint64_t t = 0; t < n_tasks; ++t) ms_task<1>(K, L, rows, frows, cr, recs, pat.data(), offs.data(), blk.data(), n_tasks, t, ptr.data(), d_steps, d_jumps);

    // the live list of ms_stage_sim: both strands of every fifth read, one strand of three of the others (by turns) and none of the fifth
    std::vector<uint64_t> live;
    std::vector<uint8_t> listed(n_tasks, 0);
    for (uint64_t r = 0; r < n_reads; ++r) {
        const uint64_t kind = (r * 7 + 3) % 5;
        if (kind == 0) { listed[2 * r] = listed[2 * r + 1] = 1; }
        else if (kind < 4) listed[2 * r + ((r + kind) & 1u)] = 1;
    }
    for (uint64_t t = 0; t < n_tasks; ++t) if (listed[t]) live.push_back(t);
    const uint64_t n_live = live.size();
    live.push_back(~0ull);                              // (what lies behind the list is not a task)

    // [0] a store per event, [1] two tasks per lane, [2] staged; [3], [4]: [1] and [2] over the live list
    const uint64_t ev_words = ws_ev_words(blk[n_blk].x, n_blk);
    EvRun R[5];
    for (int v = 0; v < 5; ++v) {
        EvRun& E = R[v];
        E.ev.assign(PAD + ev_words + PAD, GUARD); E.cnt.assign(PAD + n_tasks + PAD, GUARD32); E.col.assign(1 + MONI_EV_STAGE_N + 1, GUARD);
        uint64_t* ev = E.ev.data() + PAD; uint32_t* cnt = E.cnt.data() + PAD;
        if (v == 0) for (uint64_t t = 0; t < n_tasks; ++t) ms_task_events<1, false>(K, L, rows, frows, cr, recs, pat.data(), offs.data(), blk.data(), n_tasks, t, ev, cnt, E.steps, E.jumps);
        if (v == 1) for (uint64_t t = 0; t < n_tasks; t += 2) ms_task_events<2, false>(K, L, rows, frows, cr, recs, pat.data(), offs.data(), blk.data(), n_tasks, t, ev, cnt, E.steps, E.jumps);
        if (v == 2) for (uint64_t t = 0; t < n_tasks; ++t) ms_task_events<1, true>(K, L, rows, frows, cr, recs, pat.data(), offs.data(), blk.data(), n_tasks, t, ev, cnt, E.steps, E.jumps, nullptr, E.col.data() + 1, 1);
        if (v == 3) for (uint64_t g = 0; g < n_live; g += 2) ms_task_events<2, false>(K, L, rows, frows, cr, recs, pat.data(), offs.data(), blk.data(), n_live, g, ev, cnt, E.steps, E.jumps, live.data());
        if (v == 4) for (uint64_t g = 0; g < n_live; ++g) ms_task_events<1, true>(K, L, rows, frows, cr, recs, pat.data(), offs.data(), blk.data(), n_live, g, ev, cnt, E.steps, E.jumps, live.data(), E.col.data() + 1, 1);
        if (E.col.front() != GUARD || E.col.back() != GUARD) FAIL("variant %d: a guard word of the stage was written", v);
    }
    if (R[0].steps != d_steps || R[0].jumps != d_jumps) FAIL("events: %llu steps, %llu jumps; ms_task %llu, %llu", R[0].steps, R[0].jumps, d_steps, d_jumps);
    for (int v = 1; v < 3; ++v)
        if (R[v].ev != R[0].ev || R[v].cnt != R[0].cnt || R[v].steps != d_steps || R[v].jumps != d_jumps) FAIL("variant %d differs from a store per event, one task per lane", v);
    if (R[3].ev != R[4].ev || R[3].cnt != R[4].cnt || R[3].steps != R[4].steps || R[3].jumps != R[4].jumps) FAIL("live list: the staged form differs from a store per event");

    // every task's list: shape, expansion against the dense words, and what no list owns
    std::map<uint32_t, uint64_t> hist;
    uint64_t n_events = 0, n_wrapped = 0;
    {
        const uint64_t* ev = R[0].ev.data() + PAD; const uint32_t* cnt = R[0].cnt.data() + PAD;
        std::vector<uint8_t> owned(ev_words, 0);
        unsigned long long live_steps = 0;
        for (uint64_t t = 0; t < n_tasks; ++t) {
            const uint32_t m = len_of(t);
            const uint64_t eb = ws_ev_base(blk.data(), t), cap = ws_ev_cap(blk.data(), t), qb = ws_ptr_base(blk.data(), t);
            if (eb % 8 || eb + cap > ev_words) FAIL("task %llu: list at word %llu with room for %llu, buffer of %llu", (unsigned long long)t, (unsigned long long)eb, (unsigned long long)cap, (unsigned long long)ev_words);
            if (listed[t]) live_steps += m;
            if (!m) { if (cnt[t] != GUARD32) FAIL("task %llu has no base and a count", (unsigned long long)t); continue; }
            const uint32_t ne = cnt[t];
            if (ne == 0 || ne > m || ne > cap) FAIL("task %llu: %u events for %u steps", (unsigned long long)t, ne, m);
            hist[ne]++; n_events += ne;
            for (uint32_t k = 0; k < ne; ++k) {
                if (owned[eb + k]) FAIL("task %llu: its list overlaps another", (unsigned long long)t);
                owned[eb + k] = 1;
                const uint32_t fk = (uint32_t)(ev[eb + k] >> MONI_EV_SHIFT);
                if (k == 0 ? fk > 1 : fk <= (uint32_t)(ev[eb + k - 1] >> MONI_EV_SHIFT)) FAIL("task %llu: event %u out of order", (unsigned long long)t, k);
                if (fk > m) FAIL("task %llu: event %u behind the last step", (unsigned long long)t, k);
            }
            uint32_t k = 0;
            for (uint32_t s = 0; s < m; ++s) {
                while (k + 1 < ne && (uint32_t)(ev[eb + k + 1] >> MONI_EV_SHIFT) <= s + 1) ++k;
                const uint64_t w = (ev[eb + k] & MONI_POS_MASK) - (uint64_t)(s + 1 - (uint32_t)(ev[eb + k] >> MONI_EV_SHIFT));
                const uint64_t want = ptr[qb + (uint64_t)s * 64u];
                if (w != want) FAIL("task %llu step %u: the list gives %llx, the dense pointer is %llx", (unsigned long long)t, s, (unsigned long long)w, (unsigned long long)want);
                if (want >> 40) ++n_wrapped;
            }
            // the live run holds the same list for a listed task and nothing for another
            const uint64_t* lev = R[3].ev.data() + PAD; const uint32_t* lcnt = R[3].cnt.data() + PAD;
            if (listed[t]) { if (lcnt[t] != ne || !std::equal(ev + eb, ev + eb + ne, lev + eb)) FAIL("live list: task %llu differs", (unsigned long long)t); }
            else if (lcnt[t] != GUARD32) FAIL("live list: unlisted task %llu has a count", (unsigned long long)t);
        }
        if (R[3].steps != live_steps) FAIL("live list: %llu steps, want %llu", R[3].steps, live_steps);
        for (int v : {0, 3}) {
            const std::vector<uint64_t>& E = R[v].ev;
            for (size_t i = 0; i < E.size(); ++i) {
                const bool own = i >= PAD && i < PAD + ev_words && owned[i - PAD];
                if (!own && E[i] != GUARD) FAIL("variant %d: word %zu of the event buffer belongs to no list and was written", v, i);
            }
            for (size_t i = 0; i < PAD; ++i) if (R[v].cnt[i] != GUARD32 || R[v].cnt[PAD + n_tasks + i] != GUARD32) FAIL("variant %d: a guard word of the counts was written", v);
        }
        for (uint64_t t = 0; t < n_tasks; ++t) if (!listed[t]) {          // (an unlisted task's room in the live run: all guards)
            const uint64_t eb = ws_ev_base(blk.data(), t), cap = ws_ev_cap(blk.data(), t);
            for (uint64_t k = 0; k < cap; ++k) if (R[3].ev[PAD + eb + k] != GUARD) FAIL("live list: room of unlisted task %llu was written", (unsigned long long)t);
        }
    }

    // ---- mem_task from both sources --------------------------------------------------------------------------------------------------------------
    const uint64_t n_text = K.n_text;
    std::vector<uint8_t> text_pad(n_text + 16, 0);
    memcpy(text_pad.data(), text.data(), n_text);
    std::vector<uint64_t> text2(n_text / 32 + 2, 0), pw(8, 0);
    mem_fast_t MF;
    MF.exc_sh = text2_exc_shift(n_text, MONI_EXC_BITS);
    std::vector<uint32_t> exc((((n_text >> MF.exc_sh) + 1) + 31) / 32 + 1, 0);
    for (uint64_t w = 0; w < text2.size(); ++w) { bool bad; text2[w] = text2_word(text_pad.data(), n_text, w, bad); if (bad) { const uint64_t b = (32 * w) >> MF.exc_sh; exc[b >> 5] |= 1u << (b & 31u); } }
    MF.text2 = text2.data(); MF.exc = exc.data(); MF.pw = pw.data(); MF.pw_stride = 1; MF.pw_words = 8;      // (reads beyond 256 bases compare bytes)
    uint64_t n_mems_all = 0, n_rewalked = 0;
    unsigned long long n_cmp_all = 0;
    for (uint32_t min_len : {8u, 25u}) {
        struct Out { std::vector<uint32_t> cnt_m, cnt_s, aux; std::vector<moni_u64x2> slots; std::vector<moni_mem_t> mems; std::vector<uint64_t> rmo; unsigned long long n_cmp = 0; uint64_t n_mems = 0; } O[3];
        for (int v = 0; v < 3; ++v) {          // 0 dense, 1 events, 2 events with the closed form over silent offsets
            Out& o = O[v];
            o.cnt_m.assign(n_tasks + 1, 0); o.cnt_s.assign(n_tasks + 1, 0);
            moni_u64x2 z; z.x = z.y = GUARD;
            o.slots.assign(n_tasks * MONI_MEM_SLOTS + 1, z);
            mem_src_events_t<false> s1; s1.ev = R[2].ev.data() + PAD; s1.ev_cnt = R[2].cnt.data() + PAD;
            mem_src_events_t<true> s2; s2.ev = s1.ev; s2.ev_cnt = s1.ev_cnt;
            for (uint64_t t = 0; t < n_tasks; ++t) {
                if (v == 0) mem_task<false>(K, MF, text_pad.data(), pat.data(), offs.data(), blk.data(), t, ptr.data(), min_len, 1, o.cnt_m.data(), o.cnt_s.data(), nullptr, nullptr, nullptr, o.slots.data(), o.n_cmp);
                if (v == 1) mem_task<false>(K, MF, text_pad.data(), pat.data(), offs.data(), blk.data(), t, nullptr, min_len, 1, o.cnt_m.data(), o.cnt_s.data(), nullptr, nullptr, nullptr, o.slots.data(), o.n_cmp, s1);
                if (v == 2) mem_task<false>(K, MF, text_pad.data(), pat.data(), offs.data(), blk.data(), t, nullptr, min_len, 1, o.cnt_m.data(), o.cnt_s.data(), nullptr, nullptr, nullptr, o.slots.data(), o.n_cmp, s2);
            }
            o.rmo.assign(n_reads + 1, 0);
            for (uint64_t r = 0; r < n_reads; ++r) o.rmo[r + 1] = o.rmo[r] + o.cnt_m[2 * r] + o.cnt_m[2 * r + 1] + 2ull * (o.cnt_s[2 * r] + o.cnt_s[2 * r + 1]);
            o.n_mems = o.rmo[n_reads];
            moni_mem_t zm; memset(&zm, 0x5E, sizeof zm);
            o.mems.assign(o.n_mems + 1, zm); o.aux.assign(o.n_mems + 1, GUARD32);
            unsigned long long dummy = 0;
            for (uint64_t t = 0; t < n_tasks; ++t) {
                if (v == 0) mem_task<true>(K, MF, text_pad.data(), pat.data(), offs.data(), blk.data(), t, ptr.data(), min_len, 1, o.cnt_m.data(), o.cnt_s.data(), o.rmo.data(), o.mems.data(), o.aux.data(), o.slots.data(), dummy);
                if (v == 1) mem_task<true>(K, MF, text_pad.data(), pat.data(), offs.data(), blk.data(), t, nullptr, min_len, 1, o.cnt_m.data(), o.cnt_s.data(), o.rmo.data(), o.mems.data(), o.aux.data(), o.slots.data(), dummy, s1);
                if (v == 2) mem_task<true>(K, MF, text_pad.data(), pat.data(), offs.data(), blk.data(), t, nullptr, min_len, 1, o.cnt_m.data(), o.cnt_s.data(), o.rmo.data(), o.mems.data(), o.aux.data(), o.slots.data(), dummy, s2);
            }
        }
        for (int v = 1; v < 3; ++v) {
            const Out& a = O[0]; const Out& b = O[v];
            if (a.cnt_m != b.cnt_m || a.cnt_s != b.cnt_s) FAIL("min_len %u, source %d: MEM counts differ from the dense source's", min_len, v);
            if (a.n_cmp != b.n_cmp) FAIL("min_len %u, source %d: %llu comparisons, the dense source makes %llu", min_len, v, b.n_cmp, a.n_cmp);
            if (memcmp(a.slots.data(), b.slots.data(), a.slots.size() * sizeof(moni_u64x2))) FAIL("min_len %u, source %d: slots differ", min_len, v);
            if (a.n_mems != b.n_mems || memcmp(a.mems.data(), b.mems.data(), a.mems.size() * sizeof(moni_mem_t)) || a.aux != b.aux) FAIL("min_len %u, source %d: MEM records differ", min_len, v);
        }
        n_mems_all += O[0].n_mems; n_cmp_all += O[0].n_cmp;
        for (uint64_t t = 0; t < n_tasks; ++t) n_rewalked += O[0].cnt_m[t] > MONI_MEM_SLOTS;
    }

    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    ok = true;
    for (uint64_t t = 0; t < n_tasks; ++t) {
        const uint64_t m = len_of(t), qb = ws_ptr_base(blk.data(), t);
        for (uint64_t i = 0; i < m; ++i) {              // the pointer of read offset i is the sample of step m - 1 - i
            const uint64_t p = ptr[qb + (m - 1 - i) * 64u];
            ok = ok && fwrite(&p, 8, 1, o) == 1;
        }
    }
    const uint64_t tail[2] = {d_steps, d_jumps};
    ok = ok && fwrite(tail, 8, 2, o) == 2;
    if (fclose(o) != 0 || !ok) return 2;
    printf("list lengths:");
    for (const auto& kv : hist) printf(" %u:%llu", kv.first, (unsigned long long)kv.second);
    printf("\nOK: %llu reads, %llu steps, %llu jumps, %llu events, %llu wrapped words, %llu of %llu tasks listed; %llu MEM slots, %llu comparisons, %llu tasks walked again\n",
           (unsigned long long)n_reads, d_steps, d_jumps, (unsigned long long)n_events, (unsigned long long)n_wrapped, (unsigned long long)n_live, (unsigned long long)n_tasks,
           (unsigned long long)n_mems_all, n_cmp_all, (unsigned long long)n_rewalked);
    return 0;
}
