// TEST HARNESS ONLY - not part of the product, never linked into libmoni_hip.so.
// Replays loc_task (locate_core.h) and sc_plan / sc_segment / sc_seg_count / sc_task_of of moni_align_amd/csrc/seqcount_core.h (the code count_kernel,
// seqcount_plan_kernel and seqcount_walk_kernel run per lane) on the host over the host copy of the index image (image.hpp): task by task, then
// segment by segment in the order of the exclusive scan, each segment finding its task as a lane of the walk does.
// Two builds of this file: the shared library the tests load (scsim_*), and - with -DSEQCOUNT_SIM_MAIN - a stand-alone program that reads an index
// and a batch from a file and writes the results to another, which is how the code runs under the address and undefined-behaviour sanitizers.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../moni_align_amd/csrc/image.hpp"
#include "../../moni_align_amd/csrc/seqcount_core.h"

struct ScSim {
    HostImage img;
    lds_tables_t L;
    sc_tabs_t T;
};

static ScSim* sim_create(const moni_flat_index_t* f) {
    ScSim* S = new ScSim();
    if (S->img.build(*f)) { fprintf(stderr, "seqcount_sim: %s\n", S->img.err.c_str()); delete S; return nullptr; }
    memcpy(S->L.code, S->img.T.code, 256);
    memcpy(S->L.compl_tab, S->img.T.compl_tab, 256);
    for (int i = 0; i < 256; ++i) S->L.c2[i] = base_acgt((uint32_t)i) ? (uint8_t)base2((uint32_t)i) : (uint8_t)4;
    memcpy(S->L.abs_run, S->img.T.abs_run, sizeof(S->L.abs_run));
    memcpy(S->L.abs_pos, S->img.T.abs_pos, sizeof(S->L.abs_pos));
    for (int i = 0; i < MONI_MAX_SIGMA; ++i) {
        S->L.rec_base[i] = S->img.K.rec_base[i]; S->L.rec_cnt[i] = S->img.K.rec_cnt[i]; S->L.hot_slot[i] = S->img.K.hot_slot[i];
        S->T.rec_base[i] = S->img.K.rec_base[i]; S->T.hot_slot[i] = S->img.K.hot_slot[i];
    }
    return S;
}

// res[n_reads * strands], counts[n_reads * strands * n_seq] (zeroed here); counters: steps, fast rows, phi steps, general steps.  Returns the number of segments.
static uint64_t sim_run(ScSim* S, const uint8_t* seq, const uint64_t* offs, uint64_t n_reads, uint32_t strands, uint64_t max_walk, moni_seqcount_res_t* res,
                        uint64_t* counts, uint64_t* counters) {
    const moni_consts_t& K = S->img.K;
    const uint64_t n_pack = 2 * n_reads, n_tasks = n_reads * strands;
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
    std::vector<uint64_t> rel(n_reads + 1);
    for (uint64_t i = 0; i <= n_reads; ++i) rel[i] = offs[i] - offs[0];
    std::vector<uint64_t> pat(blk[n_blk].y + 1);
    // pack_task reads aligned 8-byte words: the device buffer is aligned and padded by 16 bytes, so is this copy
    std::vector<uint64_t> seq_pad((rel[n_reads] + 16 + 7) / 8 + 1, 0);
    if (rel[n_reads]) memcpy(seq_pad.data(), seq + offs[0], rel[n_reads]);
    const uint8_t* sq = reinterpret_cast<const uint8_t*>(seq_pad.data());
    for (uint64_t t = 0; t < n_pack; ++t) pack_task(S->L, sq, rel.data(), blk.data(), t, pat.data());
    loc_counts_t N; N.steps = N.rows = N.general = N.phi = 0;
    std::vector<uint64_t> toe(n_tasks + 1), off(n_tasks + 1, 0);
    std::vector<uint32_t> k_lo(n_tasks + 1);
    for (uint64_t t = 0; t < n_tasks; ++t) {          // count_kernel, then seqcount_plan_kernel
        moni_locate_res_t I;
        loc_task(K, S->L, S->img.rows.data(), S->img.frows.data(), S->img.cr.data(), S->img.recs.data(), pat.data(), rel.data(), blk.data(), strands == 2 ? t >> 1 : t,
                 strands == 2 ? (uint32_t)t & 1u : 0u, 0u, I, toe[t], N);
        moni_seqcount_res_t& R = res[t];
        R.count = I.count; R.sa_lo = I.sa_lo; R.matched = I.matched; R.n_seqs = 0;
        sc_plan(K, S->img.rows.data(), I.count, I.sa_lo, max_walk, k_lo[t], R.n_segs, R.walked);
        off[t + 1] = off[t] + R.n_segs;
    }
    const uint64_t total = off[n_tasks], n_seq = K.n_seq;
    for (uint64_t i = 0; i < n_tasks * n_seq; ++i) counts[i] = 0;
    phi_tab_t P; P.recs = S->img.phi.data(); P.dir = S->img.phi_dir.data();
    unsigned long long n_phi = 0;
    for (uint64_t g = 0; g < total; ++g) {             // seqcount_walk_kernel, one lane per segment
        const uint64_t t = sc_task_of(off.data(), n_tasks, g);
        const moni_seqcount_res_t& R = res[t];
        const sc_seg_t G = sc_segment(K, S->T, S->img.rows.data(), S->img.cr.data(), S->img.recs.data(), R.sa_lo, R.count, toe[t], k_lo[t], R.n_segs, (uint32_t)(g - off[t]));
        uint64_t* row = counts + t * n_seq;
        sc_seg_count(K, P, S->img.seq_starts.data(), G, n_phi, [&](uint32_t sid, uint64_t v) { row[sid] += v; });
    }
    for (uint64_t t = 0; t < n_tasks; ++t) {           // seqcount_finish_kernel
        if (!res[t].n_segs) continue;
        uint32_t k = 0;
        for (uint64_t s = 0; s < n_seq; ++s) k += counts[t * n_seq + s] != 0;
        res[t].n_seqs = k;
    }
    counters[0] = N.steps; counters[1] = N.rows; counters[2] = n_phi; counters[3] = N.general;
    return total;
}

#ifndef SEQCOUNT_SIM_MAIN

extern "C" {
void* scsim_create(const moni_flat_index_t* f) { return sim_create(f); }
void scsim_destroy(void* s) { delete (ScSim*)s; }
uint32_t scsim_n_seq(void* s) { return ((ScSim*)s)->img.K.n_seq; }
uint64_t scsim_run(void* s, const uint8_t* seq, const uint64_t* offs, uint64_t n_reads, uint32_t strands, uint64_t max_walk, moni_seqcount_res_t* res, uint64_t* counts,
                   uint64_t* counters) {
    return sim_run((ScSim*)s, seq, offs, n_reads, strands, max_walk, res, counts, counters);
}
}  // extern "C"

#else

// in:  8 u64 (n, r, w, n_seq, has_lcp, n_reads, strands, max_walk), F[256], starts[r + 1], ssa[r], esa[r], thr[r], slcp[r] if has_lcp, seq_starts[n_seq + 1],
//      offs[n_reads + 1] (u64 each), then heads[r] and the patterns' bytes
// out: res[n_tasks] (32 bytes each), counts[n_tasks * n_seq], counters[4], the number of segments (u64 each)
template <class Tp>
static bool rd(FILE* f, std::vector<Tp>& v, size_t n) { v.resize(n); return !n || fread(v.data(), sizeof(Tp), n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint64_t> h, F, starts, ssa, esa, thr, slcp, seq_starts, offs;
    std::vector<uint8_t> heads, seq;
    bool ok = rd(f, h, 8);
    if (ok) {
        const uint64_t r = h[1];
        ok = rd(f, F, 256) && rd(f, starts, r + 1) && rd(f, ssa, r) && rd(f, esa, r) && rd(f, thr, r) && (!h[4] || rd(f, slcp, r)) && rd(f, seq_starts, h[3] + 1) &&
             rd(f, offs, h[5] + 1) && rd(f, heads, r) && rd(f, seq, offs.empty() ? 0 : offs.back());
    }
    fclose(f);
    if (!ok) { fprintf(stderr, "seqcount_sim: short input\n"); return 2; }
    moni_flat_index_t fi;
    memset(&fi, 0, sizeof fi);
    fi.n = h[0]; fi.r = h[1]; fi.w = h[2]; fi.n_seq = h[3];
    fi.F = F.data(); fi.heads = heads.data(); fi.starts = starts.data(); fi.ssa = ssa.data(); fi.esa = esa.data(); fi.thr = thr.data();
    fi.slcp = h[4] ? slcp.data() : nullptr; fi.seq_starts = seq_starts.data();
    ScSim* S = sim_create(&fi);
    if (!S) return 3;
    const uint64_t n_tasks = h[5] * h[6], n_seq = h[3];
    std::vector<moni_seqcount_res_t> res(n_tasks);
    std::vector<uint64_t> counts(n_tasks * n_seq), tail(5);
    seq.resize(seq.size() + 8, 0);
    tail[4] = sim_run(S, seq.data(), offs.data(), h[5], (uint32_t)h[6], h[7], res.data(), counts.data(), tail.data());
    delete S;
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    ok = (!n_tasks || fwrite(res.data(), sizeof(moni_seqcount_res_t), n_tasks, o) == n_tasks) && (counts.empty() || fwrite(counts.data(), 8, counts.size(), o) == counts.size()) &&
         fwrite(tail.data(), 8, 5, o) == 5;
    return fclose(o) == 0 && ok ? 0 : 2;
}

#endif
