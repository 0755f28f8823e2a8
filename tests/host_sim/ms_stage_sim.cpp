// TEST HARNESS ONLY - not part of the product, never linked into libmoni_hip.so.
// A program of its own (tests/test_host_ms_stage.py builds it plain and with the address and undefined-behaviour sanitizers) over the host copy of
// the index image, with the batch laid out as moni_reads_upload and pack_kernel lay it out, for the two store forms of moni_align_amd/csrc/seed_core.h:
//  * ms_task without a live list (every task stores its own 8 bytes) against ms_task over a live list, for one and for two tasks per lane: a listed
//    task whose sister strand is not listed stores 16 bytes over both.  Every listed task's words must be the unfiltered run's, an unlisted task
//    with a listed sister holds that sister's words, and every other word of the workspace stays as it was.
//  * run_seed (what occ_task runs per seed) with a stage of OCC_STAGE_N words and without one, from many start positions, at list capacities on both
//    sides of the stage's size and with the per-genome second walk: the same list, counts and last occurrence, nothing written past the capacity.
//
// in:  8 u64 (n, r, w, n_seq, has_lcp = 1, n_reads, 0, 0), F[256], starts[r + 1], ssa[r], esa[r], thr[r], slcp[r], seq_starts[n_seq + 1],
//      offs[n_reads + 1] (u64 each), then heads[r] and the reads' bytes
// out: per read its pointers of strand 0, then those of strand 1 (the order of moni_ms_query_batch), then steps and jumps (u64 each)
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../moni_align_amd/csrc/image.hpp"
#include "../../moni_align_amd/csrc/seed_core.h"

template <class Tp>
static bool rd(FILE* f, std::vector<Tp>& v, size_t n) { v.resize(n); return !n || fread(v.data(), sizeof(Tp), n, f) == n; }

static const uint64_t FILL = 0xA5A5A5A5A5A5A5A5ull, GUARD = 0x5EED5EED5EED5EEDull;

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
    if (!ok) { fprintf(stderr, "ms_stage_sim: short input\n"); return 2; }
    moni_flat_index_t fi;
    memset(&fi, 0, sizeof fi);
    fi.n = h[0]; fi.r = h[1]; fi.w = h[2]; fi.n_seq = h[3];
    fi.F = F.data(); fi.heads = heads.data(); fi.starts = starts.data(); fi.ssa = ssa.data(); fi.esa = esa.data(); fi.thr = thr.data();
    fi.slcp = h[4] ? slcp.data() : nullptr; fi.seq_starts = seq_starts.data();
    HostImage img;
    if (img.build(fi)) { fprintf(stderr, "ms_stage_sim: %s\n", img.err.c_str()); return 3; }
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

    const moni_row_t* rows = img.rows.data(); const moni_frow_t* frows = img.frows.data(); const uint32_t* cr = img.cr.data(); const moni_rec_t* recs = img.recs.data();
    // [0] every task, one per lane; [1] every task, two per lane; [2], [3] the same over a live list that holds both strands of every fifth read, one
    // strand of three of the others (by turns) and none of the fifth
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
    std::vector<uint64_t> ptr[4];
    unsigned long long cnt[4][2];
    for (int v = 0; v < 4; ++v) {
        ptr[v].assign(blk[n_blk].x, FILL);
        cnt[v][0] = cnt[v][1] = 0;
        if (v == 0) for (uint64_t t = 0; t < n_tasks; ++t) ms_task<1>(K, L, rows, frows, cr, recs, pat.data(), offs.data(), blk.data(), n_tasks, t, ptr[v].data(), cnt[v][0], cnt[v][1]);
        if (v == 1) for (uint64_t t = 0; t < n_tasks; t += 2) ms_task<2>(K, L, rows, frows, cr, recs, pat.data(), offs.data(), blk.data(), n_tasks, t, ptr[v].data(), cnt[v][0], cnt[v][1]);
        if (v == 2) for (uint64_t g = 0; g < n_live; ++g) ms_task<1>(K, L, rows, frows, cr, recs, pat.data(), offs.data(), blk.data(), n_live, g, ptr[v].data(), cnt[v][0], cnt[v][1], live.data());
        if (v == 3) for (uint64_t g = 0; g < n_live; g += 2) ms_task<2>(K, L, rows, frows, cr, recs, pat.data(), offs.data(), blk.data(), n_live, g, ptr[v].data(), cnt[v][0], cnt[v][1], live.data());
    }
    if (cnt[1][0] != cnt[0][0] || cnt[1][1] != cnt[0][1] || ptr[1] != ptr[0]) { printf("FAIL: two tasks per lane differ from one\n"); return 1; }
    if (cnt[3][0] != cnt[2][0] || cnt[3][1] != cnt[2][1] || ptr[3] != ptr[2]) { printf("FAIL: live list, two tasks per lane differ from one\n"); return 1; }
    {
        std::vector<uint64_t> want(blk[n_blk].x, FILL);
        unsigned long long steps = 0;
        for (uint64_t t = 0; t < n_tasks; ++t) {
            const uint64_t m = offs[(t >> 1) + 1] - offs[t >> 1];
            const uint64_t from = listed[t] ? t : listed[t ^ 1] ? (t ^ 1) : ~0ull;      // whose words the task's slots hold
            if (listed[t]) steps += m;
            if (from == ~0ull) continue;
            for (uint64_t s = 0; s < m; ++s) want[ws_ptr_base(blk.data(), t) + s * 64u] = ptr[0][ws_ptr_base(blk.data(), from) + s * 64u];
        }
        if (cnt[2][0] != steps) { printf("FAIL: live list: %llu steps, want %llu\n", cnt[2][0], steps); return 1; }
        for (size_t i = 0; i < want.size(); ++i)
            if (ptr[2][i] != want[i]) { printf("FAIL: live list, workspace word %zu: %llx, want %llx\n", i, (unsigned long long)ptr[2][i], (unsigned long long)want[i]); return 1; }
    }

    // ---- run_seed with and without a stage -----------------------------------------------------------------------------------------------------
    uint64_t n_walks = 0, n_kept = 0, n_second = 0;
    {
        std::vector<uint32_t> name_id(K.n_seq);
        for (uint32_t i = 0; i < K.n_seq; ++i) name_id[i] = i;
        std::vector<uint8_t> text(K.n_text + 16, 0);
        occ_args_t A;
        memset((void*)&A, 0, sizeof A);
        A.text = text.data();
        A.phi.recs = img.phi.data(); A.phi.dir = img.phi_dir.data();
        A.phi_inv.recs = img.phi_inv.data(); A.phi_inv.dir = img.phi_inv_dir.data();
        A.seq_starts = img.seq_starts.data(); A.name_id = name_id.data();
        uint32_t small[2] = {0, 0};
        std::vector<uint32_t> pool(4 * (size_t)K.n_seq);
        A.pool_rows = 4; A.pool = pool.data(); A.pool_next = &small[0]; A.error_flag = &small[1];
        const uint32_t caps[] = {1, 4, 7, 8, 9, 12, 16, 17, 40};
        std::vector<uint64_t> col(1 + OCC_STAGE_N + 1, GUARD);
        for (uint64_t k = 0; k < fi.r; k += 1 + fi.r / 400) {
            const uint64_t pos = ssa[k];
            for (uint64_t len = 6; len <= 14; len += 4)
                for (uint32_t cap : caps)
                    for (uint32_t thr = 0; thr < 3; ++thr) {             // 0: no per-genome filter; 1, 2: at most that many per genome, the second walk
                        A.filter_seeds = thr ? 1u : 0u; A.n_seeds_thr = thr;
                        std::vector<uint64_t> out[2];
                        walk_t W[2];
                        uint64_t up[2], lo[2];
                        for (int v = 0; v < 2; ++v) {
                            out[v].assign(cap + 1, GUARD);          // exactly the capacity and a guard word behind it
                            W[v].phi_steps = 0;
                            if (v) { W[v].stage = col.data() + 1; W[v].stage_stride = 1; }
                            small[0] = small[1] = 0;
                            run_seed(A, K, pos, pos, pos, len, out[v].data(), cap, W[v], up[v], lo[v]);
                            if (small[1]) { printf("FAIL: counter pool\n"); return 1; }
                        }
                        const uint64_t n_list = std::min<uint64_t>(W[0].kept, cap);      // (what lies behind the list is the first walk's, when a second walk kept less: nobody reads it)
                        if (!std::equal(out[0].begin(), out[0].begin() + n_list, out[1].begin()) || out[0][cap] != GUARD || out[1][cap] != GUARD || W[0].kept != W[1].kept || W[0].total != W[1].total || W[0].filtered != W[1].filtered ||
                            W[0].last_kept != W[1].last_kept || up[0] != up[1] || lo[0] != lo[1] || W[0].phi_steps != W[1].phi_steps) {
                            printf("FAIL: run_seed from %llu, len %llu, cap %u, thr %u: staged and direct differ (kept %llu / %llu)\n", (unsigned long long)pos, (unsigned long long)len, cap, thr,
                                   (unsigned long long)W[1].kept, (unsigned long long)W[0].kept);
                            return 1;
                        }
                        ++n_walks; n_kept += W[0].kept; n_second += W[0].names != nullptr;
                    }
        }
        if (col.front() != GUARD || col.back() != GUARD) { printf("FAIL: a guard word of the stage was written\n"); return 1; }
    }
    uint64_t written = 0;
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    ok = true;
    for (uint64_t t = 0; t < n_tasks; ++t) {
        const uint64_t m = offs[(t >> 1) + 1] - offs[t >> 1], qb = ws_ptr_base(blk.data(), t);
        for (uint64_t i = 0; i < m; ++i) {              // the pointer of read offset i is the sample of step m - 1 - i
            const uint64_t p = ptr[0][qb + (m - 1 - i) * 64u];
            ok = ok && fwrite(&p, 8, 1, o) == 1;
            ++written;
        }
    }
    const uint64_t tail[2] = {cnt[0][0], cnt[0][1]};
    ok = ok && fwrite(tail, 8, 2, o) == 2;
    if (fclose(o) != 0 || !ok) return 2;
    printf("OK: %llu reads, %llu workspace words, %llu of %llu tasks listed, %llu steps, %llu jumps; %llu walks, %llu kept occurrences, %llu second walks\n", (unsigned long long)n_reads,
           (unsigned long long)ptr[0].size(), (unsigned long long)n_live, (unsigned long long)n_tasks, cnt[0][0], cnt[0][1], (unsigned long long)n_walks, (unsigned long long)n_kept,
           (unsigned long long)n_second);
    return 0;
}
