// TEST HARNESS ONLY - not part of the product, never linked into libmoni_hip.so.
// Replays pml_task of moni_align_amd/csrc/pml_core.h (the code pml_kernel runs per lane) read by read on the host over the host copy of the
// index image (image.hpp), with the batch laid out as moni_reads_upload and pack_kernel lay it out; beside it the pointer walk (ms_task) of
// strand 0 of the same reads, whose step and jump counts the PML walk must repeat.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../moni_align_amd/csrc/image.hpp"
#include "../../moni_align_amd/csrc/pml_core.h"

struct PmlSim {
    HostImage img;
    lds_tables_t L;
};

extern "C" {

void* pmlsim_create(const moni_flat_index_t* f) {
    PmlSim* S = new PmlSim();
    if (S->img.build(*f)) { fprintf(stderr, "pml_sim: %s\n", S->img.err.c_str()); delete S; return nullptr; }
    memcpy(S->L.code, S->img.T.code, 256);
    memcpy(S->L.compl_tab, S->img.T.compl_tab, 256);
    for (int i = 0; i < 256; ++i) S->L.c2[i] = base_acgt((uint32_t)i) ? (uint8_t)base2((uint32_t)i) : (uint8_t)4;
    memcpy(S->L.abs_run, S->img.T.abs_run, sizeof(S->L.abs_run));
    memcpy(S->L.abs_pos, S->img.T.abs_pos, sizeof(S->L.abs_pos));
    for (int i = 0; i < MONI_MAX_SIGMA; ++i) { S->L.rec_base[i] = S->img.K.rec_base[i]; S->L.rec_cnt[i] = S->img.K.rec_cnt[i]; S->L.hot_slot[i] = S->img.K.hot_slot[i]; }
    return S;
}
void pmlsim_destroy(void* s) { delete (PmlSim*)s; }

// lens[offs[i] - offs[0] + k], read_max[i], read_hits[i]; counters[0..1] = steps and jumps of the PML walk, [2..3] = those of the pointer walk of strand 0
int pmlsim_run(void* s, const uint8_t* seq, const uint64_t* offs, uint64_t n_reads, uint32_t thr, uint32_t* lens, uint32_t* read_max, uint32_t* read_hits,
               uint64_t* counters) {
    PmlSim* S = (PmlSim*)s;
    const moni_consts_t& K = S->img.K;
    const uint64_t n_tasks = 2 * n_reads;
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
    std::vector<uint64_t> pat(blk[n_blk].y + 1), ptr(blk[n_blk].x + 1);
    // pack_task reads aligned 8-byte words: the device buffer is aligned and padded by 16 bytes, so is this copy
    std::vector<uint64_t> seq_pad((rel[n_reads] + 16 + 7) / 8 + 1, 0);
    if (rel[n_reads]) memcpy(seq_pad.data(), seq + offs[0], rel[n_reads]);
    const uint8_t* sq = reinterpret_cast<const uint8_t*>(seq_pad.data());
    for (uint64_t t = 0; t < n_tasks; ++t) pack_task(S->L, sq, rel.data(), blk.data(), t, pat.data());
    unsigned long long cnt[4] = {0, 0, 0, 0};
    for (uint64_t r = 0; r < n_reads; ++r)
        pml_task(K, S->L, S->img.rows.data(), S->img.frows.data(), S->img.cr.data(), S->img.recs.data(), pat.data(), rel.data(), blk.data(), r, thr, lens, read_max, read_hits,
                 cnt[0], cnt[1]);
    for (uint64_t r = 0; r < n_reads; ++r)
        ms_task<1>(K, S->L, S->img.rows.data(), S->img.frows.data(), S->img.cr.data(), S->img.recs.data(), pat.data(), rel.data(), blk.data(), n_tasks, 2 * r, ptr.data(),
                   cnt[2], cnt[3]);
    for (int i = 0; i < 4; ++i) counters[i] = cnt[i];
    return MONI_OK;
}

}  // extern "C"
