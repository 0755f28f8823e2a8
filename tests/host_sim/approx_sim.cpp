// TEST HARNESS ONLY - not part of the product, never linked into libmoni_hip.so.
// Replays apx_exact / apx_piece / apx_task_of of moni_align_amd/csrc/approx_core.h (the code approx_exact_kernel and approx_tree_kernel run per lane)
// and loc_walk (locate_core.h) on the host over the host copy of the index image (image.hpp), the passes in launch order: the chunk counts and their
// scan, every task's exact path, every chunk as a lane of its own that finds its task over the scan, the kept counts and their scan, the gather, the
// position walks, the sort of the fetch.
// Two builds of this file: the shared library the tests load (apxsim_*), and - with -DAPPROX_SIM_MAIN - a stand-alone program that reads an index
// and a batch from a file and writes the results to another, which is how the code runs under the address and undefined-behaviour sanitizers.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../moni_align_amd/csrc/image.hpp"
#include "../../moni_align_amd/csrc/approx_core.h"

struct ApxSim {
    HostImage img;
    lds_tables_t L;
    std::vector<moni_approx_res_t> res;
    std::vector<moni_approx_hit_t> hits;
    std::vector<uint64_t> pos, seq_off;
    std::vector<uint32_t> seq;
    uint64_t counters[4];
};

static ApxSim* sim_create(const moni_flat_index_t* f) {
    ApxSim* S = new ApxSim();
    if (S->img.build(*f)) { fprintf(stderr, "approx_sim: %s\n", S->img.err.c_str()); delete S; return nullptr; }
    memcpy(S->L.code, S->img.T.code, 256);
    memcpy(S->L.compl_tab, S->img.T.compl_tab, 256);
    for (int i = 0; i < 256; ++i) S->L.c2[i] = base_acgt((uint32_t)i) ? (uint8_t)base2((uint32_t)i) : (uint8_t)4;
    memcpy(S->L.abs_run, S->img.T.abs_run, sizeof(S->L.abs_run));
    memcpy(S->L.abs_pos, S->img.T.abs_pos, sizeof(S->L.abs_pos));
    for (int i = 0; i < MONI_MAX_SIGMA; ++i) { S->L.rec_base[i] = S->img.K.rec_base[i]; S->L.rec_cnt[i] = S->img.K.rec_cnt[i]; S->L.hot_slot[i] = S->img.K.hot_slot[i]; }
    return S;
}

// prm: strands, k, max_hits, max_occ, chunk_len, max_steps.  The results stay in S (sim_fetch-style accessors below).
static void sim_run(ApxSim* S, const uint8_t* seq, const uint64_t* offs, uint64_t n_reads, const uint64_t* prm) {
    const moni_consts_t& K = S->img.K;
    const uint32_t strands = (uint32_t)prm[0], k = (uint32_t)prm[1], max_hits = (uint32_t)prm[2], max_occ = (uint32_t)prm[3], chunk_len = (uint32_t)prm[4];
    const uint64_t n_pack = 2 * n_reads, n_tasks = n_reads * strands;
    // the workspace layout of reads_upload (moni_hip.hip): per block of 32 reads as many steps as its longest read has
    const uint64_t n_blk = (n_reads + 31) / 32;
    std::vector<moni_u64x2> blk(n_blk + 1);
    {
        uint64_t pw = 0, qw = 0;
        for (uint64_t b = 0; b < n_blk; ++b) {
            uint64_t lb = 0;
            for (uint64_t i = 32 * b; i < n_reads && i < 32 * b + 32; ++i) lb = std::max<uint64_t>(lb, offs[i + 1] - offs[i]);
            blk[b].x = qw; blk[b].y = pw;
            qw += 64 * lb; pw += 64 * ws_pat_words(lb);
        }
        blk[n_blk].x = qw; blk[n_blk].y = pw;
    }
    std::vector<uint64_t> rel(n_reads + 1);
    for (uint64_t i = 0; i <= n_reads; ++i) rel[i] = offs[i] - offs[0];
    std::vector<uint64_t> pat(blk[n_blk].y + 1);
    // pack_task reads aligned 8-byte words: the device buffer is aligned and padded by 16 bytes, so is this copy
    std::vector<uint64_t> seq_pad((rel[n_reads] + 16 + 7) / 8 + 1, 0);
    if (rel[n_reads]) memcpy(seq_pad.data(), seq + offs[0], rel[n_reads]);
    const uint8_t* sq = reinterpret_cast<const uint8_t*>(seq_pad.data());
    for (uint64_t t = 0; t < n_pack; ++t) pack_task(S->L, sq, rel.data(), blk.data(), t, pat.data());

    S->res.assign(n_tasks, moni_approx_res_t());
    std::vector<moni_approx_hit_t> slots(n_tasks * max_hits);
    apx_args_t A;
    A.rows = S->img.rows.data(); A.frows = S->img.frows.data(); A.cr = S->img.cr.data(); A.recs = S->img.recs.data(); A.pat = pat.data(); A.offs = rel.data(); A.blk = blk.data();
    A.strands = strands; A.k = k; A.max_hits = max_hits; A.max_occ = max_occ; A.chunk_len = chunk_len; A.max_steps = prm[5];
    A.res = S->res.data(); A.slots = slots.data();
    std::vector<uint64_t> ck_off(n_tasks + 1, 0);
    if (k) for (uint64_t t = 0; t < n_tasks; ++t) {          // approx_plan_kernel and the scan
        const uint64_t read = strands == 2 ? t >> 1 : t;
        ck_off[t + 1] = ck_off[t] + apx_n_chunks((uint32_t)(rel[read + 1] - rel[read]), chunk_len);
    }
    std::vector<apx_ckpt_t> ckpt(ck_off[n_tasks]);            // exactly the chunks: a checkpoint written past them is a heap overflow the sanitizer sees
    loc_counts_t N; N.steps = N.rows = N.general = N.phi = 0;
    for (uint64_t t = 0; t < n_tasks; ++t) apx_exact(K, S->L, A, t, k ? ckpt.data() + ck_off[t] : nullptr, N);          // approx_exact_kernel
    unsigned long long rewalk = 0;
    if (k) for (uint64_t g = 0; g < ck_off[n_tasks]; ++g) {   // approx_tree_kernel, one lane per chunk
        const uint64_t t = apx_task_of(ck_off.data(), n_tasks, g);
        uint64_t stack[APX_STACK_LEVELS * APX_STACK_WORDS];
        apx_piece(K, S->L, A, t, g - ck_off[t], ckpt.data() + ck_off[t], stack, 1, N, rewalk);
    }
    S->hits.clear(); S->pos.clear(); S->seq.clear(); S->seq_off.clear();
    std::vector<uint64_t> toes;
    for (uint64_t t = 0; t < n_tasks && max_hits; ++t) {      // approx_finish_kernel, the scan, approx_gather_kernel
        moni_approx_res_t& R = S->res[t];
        R.n_kept = std::min(R.n_kept, max_hits);
        R.hit_off = S->hits.size();
        for (uint32_t j = 0; j < R.n_kept; ++j) { S->hits.push_back(slots[t * max_hits + j]); toes.push_back(slots[t * max_hits + j].occ_off); S->hits.back().occ_off = 0; }
    }
    phi_tab_t P; P.recs = S->img.phi.data(); P.dir = S->img.phi_dir.data();
    if (max_occ) for (size_t h = 0; h < S->hits.size(); ++h) {    // the scan of n_occ, approx_walk_kernel
        const uint64_t o = S->pos.size(), n = S->hits[h].n_occ;
        S->pos.resize(o + n); S->seq.resize(o + n); S->seq_off.resize(o + n);
        S->hits[h].occ_off = o;
        if (n) loc_walk(K, P, S->img.seq_starts.data(), toes[h], (uint32_t)n, S->pos.data() + o, S->seq.data() + o, S->seq_off.data() + o, N);
    }
    // moni_approx_fetch: the hits of a task in their order, the positions behind them
    if (!S->hits.empty()) {
        apx_sort_hits(S->hits.data(), S->res.data(), n_tasks);
        std::vector<uint64_t> tp = S->pos, to = S->seq_off; std::vector<uint32_t> ts = S->seq;
        uint64_t at = 0;
        for (auto& H : S->hits) {
            std::copy(tp.begin() + H.occ_off, tp.begin() + H.occ_off + H.n_occ, S->pos.begin() + at);
            std::copy(ts.begin() + H.occ_off, ts.begin() + H.occ_off + H.n_occ, S->seq.begin() + at);
            std::copy(to.begin() + H.occ_off, to.begin() + H.occ_off + H.n_occ, S->seq_off.begin() + at);
            H.occ_off = at; at += H.n_occ;
        }
    }
    S->counters[0] = N.steps - rewalk; S->counters[1] = N.rows; S->counters[2] = N.phi; S->counters[3] = N.general;
}

#ifndef APPROX_SIM_MAIN

extern "C" {
void* apxsim_create(const moni_flat_index_t* f) { return sim_create(f); }
void apxsim_destroy(void* s) { delete (ApxSim*)s; }
// sizes: n_tasks, kept hits, positions
void apxsim_run(void* s, const uint8_t* seq, const uint64_t* offs, uint64_t n_reads, const uint64_t* prm, uint64_t* sizes) {
    ApxSim* S = (ApxSim*)s;
    sim_run(S, seq, offs, n_reads, prm);
    sizes[0] = S->res.size(); sizes[1] = S->hits.size(); sizes[2] = S->pos.size();
}
void apxsim_fetch(void* s, moni_approx_res_t* res, moni_approx_hit_t* hits, uint64_t* pos, uint32_t* seq, uint64_t* seq_off, uint64_t* counters) {
    ApxSim* S = (ApxSim*)s;
    std::copy(S->res.begin(), S->res.end(), res);
    std::copy(S->hits.begin(), S->hits.end(), hits);
    std::copy(S->pos.begin(), S->pos.end(), pos);
    std::copy(S->seq.begin(), S->seq.end(), seq);
    std::copy(S->seq_off.begin(), S->seq_off.end(), seq_off);
    std::copy(S->counters, S->counters + 4, counters);
}
}  // extern "C"

#else

// in:  14 u64 (n, r, w, n_seq, has_lcp, n_reads, strands, k, max_hits, max_occ, chunk_len, max_steps, 0, 0), F[256], starts[r + 1], ssa[r], esa[r], thr[r],
//      slcp[r] if has_lcp, seq_starts[n_seq + 1], offs[n_reads + 1] (u64 each), then heads[r] and the patterns' bytes
// out: 8 u64 (n_tasks, hits, positions, counters[4], 0), res (64 bytes each), hits (40 bytes each), pos (u64), seq_off (u64), seq (u32)
template <class Tp>
static bool rd(FILE* f, std::vector<Tp>& v, size_t n) { v.resize(n); return !n || fread(v.data(), sizeof(Tp), n, f) == n; }
template <class Tp>
static bool wr(FILE* f, const std::vector<Tp>& v) { return v.empty() || fwrite(v.data(), sizeof(Tp), v.size(), f) == v.size(); }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint64_t> h, F, starts, ssa, esa, thr, slcp, seq_starts, offs;
    std::vector<uint8_t> heads, seq;
    bool ok = rd(f, h, 14);
    if (ok) {
        const uint64_t r = h[1];
        ok = rd(f, F, 256) && rd(f, starts, r + 1) && rd(f, ssa, r) && rd(f, esa, r) && rd(f, thr, r) && (!h[4] || rd(f, slcp, r)) && rd(f, seq_starts, h[3] + 1) &&
             rd(f, offs, h[5] + 1) && rd(f, heads, r) && rd(f, seq, offs.empty() ? 0 : offs.back());
    }
    fclose(f);
    if (!ok) { fprintf(stderr, "approx_sim: short input\n"); return 2; }
    moni_flat_index_t fi;
    memset(&fi, 0, sizeof fi);
    fi.n = h[0]; fi.r = h[1]; fi.w = h[2]; fi.n_seq = h[3];
    fi.F = F.data(); fi.heads = heads.data(); fi.starts = starts.data(); fi.ssa = ssa.data(); fi.esa = esa.data(); fi.thr = thr.data();
    fi.slcp = h[4] ? slcp.data() : nullptr; fi.seq_starts = seq_starts.data();
    ApxSim* S = sim_create(&fi);
    if (!S) return 3;
    seq.resize(seq.size() + 8, 0);
    sim_run(S, seq.data(), offs.data(), h[5], h.data() + 6);
    std::vector<uint64_t> head = {S->res.size(), S->hits.size(), S->pos.size(), S->counters[0], S->counters[1], S->counters[2], S->counters[3], 0};
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); delete S; return 2; }
    ok = wr(o, head) && wr(o, S->res) && wr(o, S->hits) && wr(o, S->pos) && wr(o, S->seq_off) && wr(o, S->seq);
    delete S;
    return fclose(o) == 0 && ok ? 0 : 2;
}

#endif
