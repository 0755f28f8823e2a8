// TEST HARNESS ONLY - not part of the product, never linked into libmoni_hip.so.
// Replays the three per-lane routines of moni_align_amd/csrc/mslong_core.h (the segment table, mslong_walk, mslong_len: what the kernels of
// mslong_kernels.hip run per lane) on the host over the host copy of the index image (image.hpp), with the lanes as loops and the rounds in the
// order moni_ms_long_batch launches them: table, speculative walk, length pass with flags, runs of flagged segments, chain re-walk, length pass.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../moni_align_amd/csrc/image.hpp"
#include "../../moni_align_amd/csrc/mslong_core.h"

struct MslSim {
    HostImage img;
    lds_tables_t L;
    std::vector<uint64_t> text;          // 8-byte aligned and padded, as the device copy
};

extern "C" {

void* mslsim_create(const moni_flat_index_t* f) {
    MslSim* S = new MslSim();
    if (S->img.build(*f)) { fprintf(stderr, "mslong_sim: %s\n", S->img.err.c_str()); delete S; return nullptr; }
    memcpy(S->L.code, S->img.T.code, 256);
    memcpy(S->L.compl_tab, S->img.T.compl_tab, 256);
    for (int i = 0; i < 256; ++i) S->L.c2[i] = base_acgt((uint32_t)i) ? (uint8_t)base2((uint32_t)i) : (uint8_t)4;
    memcpy(S->L.abs_run, S->img.T.abs_run, sizeof(S->L.abs_run));
    memcpy(S->L.abs_pos, S->img.T.abs_pos, sizeof(S->L.abs_pos));
    for (int i = 0; i < MONI_MAX_SIGMA; ++i) { S->L.rec_base[i] = S->img.K.rec_base[i]; S->L.rec_cnt[i] = S->img.K.rec_cnt[i]; S->L.hot_slot[i] = S->img.K.hot_slot[i]; }
    const uint64_t nt = S->img.K.n_text;
    S->text.assign((nt + 16 + 7) / 8 + 1, 0);
    if (!f->text) { fprintf(stderr, "mslong_sim: the index has no text\n"); delete S; return nullptr; }
    memcpy(S->text.data(), f->text, nt);
    return S;
}
void mslsim_destroy(void* s) { delete (MslSim*)s; }

// pointers[offs[i] - offs[0] + k], lengths[...]; stats[0..5] = segments, flagged, chain_runs, steps_spec, steps_chain, jumps;
// segs_out (may be NULL): the first segs_cap rows of the segment table as (pattern, a, b, e)
int mslsim_run(void* s, const uint8_t* seq, const uint64_t* offs, uint64_t n_pat, uint32_t seg_len, uint32_t overlap, uint64_t* pointers, uint32_t* lengths,
               uint64_t* stats, uint32_t* segs_out, uint64_t segs_cap) {
    MslSim* S = (MslSim*)s;
    const moni_consts_t& K = S->img.K;
    std::vector<uint64_t> rel(n_pat + 1);
    for (uint64_t i = 0; i <= n_pat; ++i) rel[i] = offs[i] - offs[0];
    const uint64_t total = rel[n_pat];
    std::vector<uint64_t> seq_pad((total + 16 + 7) / 8 + 1, 0);
    if (total) memcpy(seq_pad.data(), seq + offs[0], total);
    const uint8_t* sq = reinterpret_cast<const uint8_t*>(seq_pad.data());
    const uint8_t* text = reinterpret_cast<const uint8_t*>(S->text.data());
    // the segment table: counts, their exclusive scan, one entry per segment found by search (mslong_count_kernel / mslong_table_kernel)
    std::vector<uint64_t> seg_off(n_pat + 1, 0);
    for (uint64_t i = 0; i < n_pat; ++i) seg_off[i + 1] = seg_off[i] + mslong_n_segs(rel[i], rel[i + 1] - rel[i], seg_len);
    const uint64_t n_segs = seg_off[n_pat];
    std::vector<mslong_seg_t> segs(n_segs);
    for (uint64_t g = 0; g < n_segs; ++g) {
        uint64_t lo = 0, hi = n_pat;
        while (hi - lo > 1) { const uint64_t mid = lo + ((hi - lo) >> 1); if (seg_off[mid] <= g) lo = mid; else hi = mid; }
        segs[g] = mslong_seg((uint32_t)lo, rel[lo], rel[lo + 1] - rel[lo], seg_len, overlap, g - seg_off[lo]);
    }
    if (segs_out) for (uint64_t g = 0; g < n_segs && g < segs_cap; ++g) { segs_out[4 * g] = segs[g].pat; segs_out[4 * g + 1] = segs[g].a; segs_out[4 * g + 2] = segs[g].b; segs_out[4 * g + 3] = segs[g].e; }
    std::vector<mslong_state_t> states(n_segs + 1);
    std::vector<uint32_t> flags(n_segs + 1, 0);
    uint32_t glo[8]; uint8_t ghi[8];
    mslong_grp_t G; G.lo = glo; G.hi = ghi; G.stride = 1;
    unsigned long long steps_spec = 0, steps_chain = 0, jumps = 0, flagged = 0;
    for (uint64_t g = 0; g < n_segs; ++g) {
        const mslong_seg_t x = segs[g];
        mslong_walk(K, S->L, S->img.rows.data(), S->img.frows.data(), S->img.cr.data(), S->img.recs.data(), sq, rel[x.pat], rel[x.pat], x.a, x.b, x.e, nullptr, pointers,
                    &states[g], G, steps_spec, jumps);
    }
    for (uint64_t g = 0; g < n_segs; ++g) {
        const mslong_seg_t x = segs[g];
        const uint32_t m = (uint32_t)(rel[x.pat + 1] - rel[x.pat]);
        const uint64_t reach = mslong_len(K, text, sq, rel[x.pat], rel[x.pat], x.a, x.b, x.e, m, pointers, lengths);
        if (x.e < m && reach >= x.e) { flags[g] = 1; ++flagged; }
    }
    std::vector<mslong_run_t> runs;
    for (uint64_t g = 0; g < n_segs; ++g) {
        if (!flags[g] || (g > 0 && flags[g - 1])) continue;
        uint64_t t = g;
        while (t + 1 < n_segs && flags[t + 1]) ++t;
        mslong_run_t r; r.s0 = (uint32_t)g; r.s1 = (uint32_t)t;
        runs.push_back(r);
    }
    for (const mslong_run_t& r : runs) {
        if ((uint64_t)r.s1 + 1 >= n_segs || segs[r.s1 + 1].pat != segs[r.s0].pat) { fprintf(stderr, "mslong_sim: a run of flagged segments ends its pattern\n"); return MONI_ERANGE; }
        const mslong_seg_t g0 = segs[r.s0], g1 = segs[r.s1];
        mslong_walk(K, S->L, S->img.rows.data(), S->img.frows.data(), S->img.cr.data(), S->img.recs.data(), sq, rel[g0.pat], rel[g0.pat], g0.a, g1.b, g1.b, &states[r.s1 + 1], pointers,
                    nullptr, G, steps_chain, jumps);
    }
    for (const mslong_run_t& r : runs) {
        const mslong_seg_t g0 = segs[r.s0], g1 = segs[r.s1];
        const uint32_t m = (uint32_t)(rel[g0.pat + 1] - rel[g0.pat]);
        (void)mslong_len(K, text, sq, rel[g0.pat], rel[g0.pat], g0.a, g1.b, m, m, pointers, lengths);
    }
    stats[0] = n_segs; stats[1] = flagged; stats[2] = runs.size(); stats[3] = steps_spec; stats[4] = steps_chain; stats[5] = jumps;
    return MONI_OK;
}

}  // extern "C"
