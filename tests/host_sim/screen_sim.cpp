// TEST HARNESS ONLY - not part of the product, never linked into libmoni_hip.so.
// Replays screen_task of moni_align_amd/csrc/screen_core.h (the code screen_kernel runs per lane) lane by lane on the host over the host copy of the
// index image (image.hpp), with the batch laid out as moni_reads_upload and pack_kernel lay it out.  The lanes of a read run one after the other in
// the order N1, P1, N0, P0: what a lane takes from its neighbours on the device with a cross-lane move it takes here from a log the neighbour
// filled when it ran - the null lane its histogram words at every window's end, strand 1's pattern lane its three figures.
// -DSCREEN_SIM_MAIN: the same as a program of its own (file in, file out), for a run under the sanitizers.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../moni_align_amd/csrc/image.hpp"
#include "../../moni_align_amd/csrc/screen_core.h"

struct ScreenSim {
    HostImage img;
    lds_tables_t L;
};

// X.pair / X.strand of screen_task for lanes that run one after the other
struct LogXchg {
    uint32_t role = 0;
    std::vector<uint32_t> pair_log, strand_log;
    size_t pair_at = 0, strand_at = 0;
    bool underrun = false;
    uint32_t pair(uint32_t v) {
        if (role & 1u) { pair_log.push_back(v); return 0; }
        if (pair_at >= pair_log.size()) { underrun = true; return 0; }
        return pair_log[pair_at++];
    }
    uint32_t strand(uint32_t v) {
        if (role == 2) { strand_log.push_back(v); return 0; }
        if (role != 0) return 0;
        if (strand_at >= strand_log.size()) { underrun = true; return 0; }
        return strand_log[strand_at++];
    }
};

static ScreenSim* sim_create(const moni_flat_index_t* f) {
    ScreenSim* S = new ScreenSim();
    if (S->img.build(*f)) { fprintf(stderr, "screen_sim: %s\n", S->img.err.c_str()); delete S; return nullptr; }
    memcpy(S->L.code, S->img.T.code, 256);
    memcpy(S->L.compl_tab, S->img.T.compl_tab, 256);
    for (int i = 0; i < 256; ++i) S->L.c2[i] = base_acgt((uint32_t)i) ? (uint8_t)base2((uint32_t)i) : (uint8_t)4;
    memcpy(S->L.abs_run, S->img.T.abs_run, sizeof(S->L.abs_run));
    memcpy(S->L.abs_pos, S->img.T.abs_pos, sizeof(S->L.abs_pos));
    for (int i = 0; i < MONI_MAX_SIGMA; ++i) { S->L.rec_base[i] = S->img.K.rec_base[i]; S->L.rec_cnt[i] = S->img.K.rec_cnt[i]; S->L.hot_slot[i] = S->img.K.hot_slot[i]; }
    return S;
}

// res[i]; counters[0..2] = steps, jumps of all lanes, jumps of the P0 lanes; [3] = 1 if a lane left its histogram column non-zero or a log ran dry
static int sim_run(ScreenSim* S, const uint8_t* seq, const uint64_t* offs, uint64_t n_reads, const moni_screen_params_t* prm, moni_screen_res_t* res, uint64_t* counters) {
    if (!prm || !screen_params_ok(*prm)) return MONI_EINVAL;
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
    std::vector<uint64_t> pat(blk[n_blk].y + 1);
    // pack_task reads aligned 8-byte words: the device buffer is aligned and padded by 16 bytes, so is this copy
    std::vector<uint64_t> seq_pad((rel[n_reads] + 16 + 7) / 8 + 1, 0);
    if (rel[n_reads]) memcpy(seq_pad.data(), seq + offs[0], rel[n_reads]);
    const uint8_t* sq = reinterpret_cast<const uint8_t*>(seq_pad.data());
    for (uint64_t t = 0; t < n_tasks; ++t) pack_task(S->L, sq, rel.data(), blk.data(), t, pat.data());
    unsigned long long cnt[3] = {0, 0, 0};
    uint64_t bad = 0;
    const uint32_t n_roles = 2 * prm->strands;
    for (uint64_t r = 0; r < n_reads; ++r) {
        LogXchg X;
        for (uint32_t k = 0; k < n_roles; ++k) {
            const uint32_t role = n_roles - 1 - k;          // N1, P1, N0, P0
            uint32_t hist[SCREEN_WORDS] = {0};
            X.role = role;
            if (role == 1) { X.pair_log.clear(); X.pair_at = 0; }          // (strand 1's words were all taken)
            screen_task(K, S->L, S->img.rows.data(), S->img.frows.data(), S->img.cr.data(), S->img.recs.data(), pat.data(), rel.data(), blk.data(), r, role, *prm, hist, 1u, X, res,
                        cnt[0], cnt[1], cnt[2]);
            for (uint32_t w = 0; w < SCREEN_WORDS; ++w) if (hist[w]) bad = 1;
            if (!(role & 1u) && X.pair_at != X.pair_log.size()) bad = 1;
        }
        if (X.underrun || X.strand_at != X.strand_log.size()) bad = 1;
    }
    for (int i = 0; i < 3; ++i) counters[i] = cnt[i];
    counters[3] = bad;
    return MONI_OK;
}

#ifndef SCREEN_SIM_MAIN

extern "C" {
void* screensim_create(const moni_flat_index_t* f) { return sim_create(f); }
void screensim_destroy(void* s) { delete (ScreenSim*)s; }
int screensim_run(void* s, const uint8_t* seq, const uint64_t* offs, uint64_t n_reads, const moni_screen_params_t* prm, moni_screen_res_t* res, uint64_t* counters) {
    return sim_run((ScreenSim*)s, seq, offs, n_reads, prm, res, counters);
}
uint32_t screensim_n_win(uint32_t m, const moni_screen_params_t* prm) { return screen_n_win(m, *prm); }
}  // extern "C"

#else

// in:  12 u64 (n, r, w, n_seq, has_lcp, n_reads, strands, window, min_win, ks_num, ks_den, 0), F[256], starts[r + 1], ssa[r], esa[r], thr[r], slcp[r] if has_lcp,
//      seq_starts[n_seq + 1], offs[n_reads + 1] (u64 each), then heads[r] and the reads' bytes
// out: res[n_reads] (32 bytes each), counters[4] (u64 each)
template <class Tp>
static bool rd(FILE* f, std::vector<Tp>& v, size_t n) { v.resize(n); return !n || fread(v.data(), sizeof(Tp), n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint64_t> h, F, starts, ssa, esa, thr, slcp, seq_starts, offs;
    std::vector<uint8_t> heads, seq;
    bool ok = rd(f, h, 12);
    if (ok) {
        const uint64_t r = h[1];
        ok = rd(f, F, 256) && rd(f, starts, r + 1) && rd(f, ssa, r) && rd(f, esa, r) && rd(f, thr, r) && (!h[4] || rd(f, slcp, r)) && rd(f, seq_starts, h[3] + 1) &&
             rd(f, offs, h[5] + 1) && rd(f, heads, r) && rd(f, seq, offs.empty() ? 0 : offs.back());
    }
    fclose(f);
    if (!ok) { fprintf(stderr, "screen_sim: short input\n"); return 2; }
    moni_flat_index_t fi;
    memset(&fi, 0, sizeof fi);
    fi.n = h[0]; fi.r = h[1]; fi.w = h[2]; fi.n_seq = h[3];
    fi.F = F.data(); fi.heads = heads.data(); fi.starts = starts.data(); fi.ssa = ssa.data(); fi.esa = esa.data(); fi.thr = thr.data();
    fi.slcp = h[4] ? slcp.data() : nullptr; fi.seq_starts = seq_starts.data();
    ScreenSim* S = sim_create(&fi);
    if (!S) return 3;
    moni_screen_params_t prm;
    memset(&prm, 0, sizeof prm);
    prm.strands = (uint32_t)h[6]; prm.window = (uint32_t)h[7]; prm.min_win = (uint32_t)h[8]; prm.ks_num = (uint32_t)h[9]; prm.ks_den = (uint32_t)h[10];
    std::vector<moni_screen_res_t> res(h[5] + 1);
    std::vector<uint64_t> tail(4);
    seq.resize(seq.size() + 8, 0);
    const int rc = sim_run(S, seq.data(), offs.data(), h[5], &prm, res.data(), tail.data());
    delete S;
    if (rc) return 4;
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    ok = (!h[5] || fwrite(res.data(), sizeof(moni_screen_res_t), h[5], o) == h[5]) && fwrite(tail.data(), 8, 4, o) == 4;
    return fclose(o) == 0 && ok ? 0 : 2;
}

#endif
