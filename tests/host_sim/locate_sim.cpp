// TEST HARNESS ONLY - not part of the product, never linked into libmoni_hip.so.
// Replays loc_task and loc_walk of moni_align_amd/csrc/locate_core.h (the code count_kernel and locate_walk_kernel run per lane) task by task on
// the host over the host copy of the index image (image.hpp), with the batch laid out as moni_reads_upload and pack_kernel lay it out and the
// offsets the exclusive scan gives.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../moni_align_amd/csrc/image.hpp"
#include "../../moni_align_amd/csrc/locate_core.h"

struct LocSim {
    HostImage img;
    lds_tables_t L;
    std::vector<uint64_t> pos, seq_off;
    std::vector<uint32_t> seq;
};

extern "C" {

void* locsim_create(const moni_flat_index_t* f) {
    LocSim* S = new LocSim();
    if (S->img.build(*f)) { fprintf(stderr, "locate_sim: %s\n", S->img.err.c_str()); delete S; return nullptr; }
    memcpy(S->L.code, S->img.T.code, 256);
    memcpy(S->L.compl_tab, S->img.T.compl_tab, 256);
    for (int i = 0; i < 256; ++i) S->L.c2[i] = base_acgt((uint32_t)i) ? (uint8_t)base2((uint32_t)i) : (uint8_t)4;
    memcpy(S->L.abs_run, S->img.T.abs_run, sizeof(S->L.abs_run));
    memcpy(S->L.abs_pos, S->img.T.abs_pos, sizeof(S->L.abs_pos));
    for (int i = 0; i < MONI_MAX_SIGMA; ++i) { S->L.rec_base[i] = S->img.K.rec_base[i]; S->L.rec_cnt[i] = S->img.K.rec_cnt[i]; S->L.hot_slot[i] = S->img.K.hot_slot[i]; }
    return S;
}
void locsim_destroy(void* s) { delete (LocSim*)s; }

// res[n_reads * strands]; the positions stay in the object (locsim_fetch); counters: steps, fast rows, phi steps, general steps.  Returns the number of positions.
uint64_t locsim_run(void* s, const uint8_t* seq, const uint64_t* offs, uint64_t n_reads, uint32_t strands, uint32_t max_occ, moni_locate_res_t* res, uint64_t* counters) {
    LocSim* S = (LocSim*)s;
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
    for (uint64_t t = 0; t < n_tasks; ++t) {
        loc_task(K, S->L, S->img.rows.data(), S->img.frows.data(), S->img.cr.data(), S->img.recs.data(), pat.data(), rel.data(), blk.data(), strands == 2 ? t >> 1 : t,
                 strands == 2 ? (uint32_t)t & 1u : 0u, max_occ, res[t], toe[t], N);
        off[t + 1] = off[t] + res[t].n_occ;
    }
    const uint64_t total = off[n_tasks];
    S->pos.assign(total + 1, 0); S->seq.assign(total + 1, 0); S->seq_off.assign(total + 1, 0);
    phi_tab_t P; P.recs = S->img.phi.data(); P.dir = S->img.phi_dir.data();
    if (total)
        for (uint64_t t = 0; t < n_tasks; ++t) {
            res[t].occ_off = off[t];
            if (res[t].n_occ) loc_walk(K, P, S->img.seq_starts.data(), toe[t], res[t].n_occ, S->pos.data() + off[t], S->seq.data() + off[t], S->seq_off.data() + off[t], N);
        }
    counters[0] = N.steps; counters[1] = N.rows; counters[2] = N.phi; counters[3] = N.general;
    return total;
}

void locsim_fetch(void* s, uint64_t n, uint64_t* pos, uint32_t* seq, uint64_t* seq_off) {
    LocSim* S = (LocSim*)s;
    if (n) { memcpy(pos, S->pos.data(), n * 8); memcpy(seq, S->seq.data(), n * 4); memcpy(seq_off, S->seq_off.data(), n * 8); }
}

}  // extern "C"
