// TEST HARNESS ONLY - not part of the product, never linked into libmoni_hip.so.
// Replays the loci query on the host over the host copy of the index image (image.hpp) and the lift tables (lift_build.hpp): loc_task
// (locate_core.h), sc_plan / sc_segment / sc_task_of (seqcount_core.h) and loci_seg_hi / loci_seg_keys / loci_key / loci_is_head of
// moni_align_amd/csrc/loci_core.h - the code count_kernel, seqcount_plan_kernel, loci_plan_kernel, loci_walk_kernel, loci_head_kernel,
// loci_emit_kernel and loci_finish_kernel run per lane - lanes as loops, passes in launch order, std::sort for the device sort.  The key buffer
// holds the walked total exactly: a slot outside it is a heap overflow the sanitizers see.
// Two builds of this file: the shared library the tests load (locisim_*), and - with -DLOCI_SIM_MAIN - a stand-alone program that reads an index
// and a batch from a file and writes the results to another, which is how the code runs under the address and undefined-behaviour sanitizers.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../moni_align_amd/csrc/image.hpp"
#include "../../moni_align_amd/csrc/lift_build.hpp"
#include "../../moni_align_amd/csrc/loci_core.h"

struct LociSim {
    HostImage img;
    LiftTables lt;
    lds_tables_t L;
    sc_tabs_t T;
    loci_lift_t lift() const {
        loci_lift_t X; X.pdir = lt.pdir.data(); X.seqs = lt.seqs.data(); X.runs = lt.runs.data(); X.n_text = img.K.n - 1; X.n_seq = img.K.n_seq;
        return X;
    }
};

struct LociOut {
    std::vector<moni_loci_res_t> res;
    std::vector<uint64_t> lpos, lseq_off, support;
    std::vector<uint32_t> lseq;
    uint64_t counters[4] = {0, 0, 0, 0}, n_segs = 0, total = 0;
};

static LociSim* sim_create(const moni_flat_index_t* f) {
    LociSim* S = new LociSim();
    std::string err;
    if (S->img.build(*f)) { fprintf(stderr, "loci_sim: %s\n", S->img.err.c_str()); delete S; return nullptr; }
    if (S->lt.build(*f, err)) { fprintf(stderr, "loci_sim: %s\n", err.c_str()); delete S; return nullptr; }
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

static void sim_run(LociSim* S, const uint8_t* seq, const uint64_t* offs, uint64_t n_reads, uint32_t strands, uint32_t lift, uint64_t max_walk, LociOut& O) {
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
    std::vector<moni_seqcount_res_t> sres(n_tasks);
    std::vector<uint64_t> toe(n_tasks + 1), off(n_tasks + 1, 0), occ_off(n_tasks + 1, 0);
    std::vector<uint32_t> k_lo(n_tasks + 1);
    for (uint64_t t = 0; t < n_tasks; ++t) {          // count_kernel, seqcount_plan_kernel, loci_plan_kernel and the two scans
        moni_locate_res_t I;
        loc_task(K, S->L, S->img.rows.data(), S->img.frows.data(), S->img.cr.data(), S->img.recs.data(), pat.data(), rel.data(), blk.data(), strands == 2 ? t >> 1 : t,
                 strands == 2 ? (uint32_t)t & 1u : 0u, 0u, I, toe[t], N);
        moni_seqcount_res_t& R = sres[t];
        R.count = I.count; R.sa_lo = I.sa_lo; R.matched = I.matched; R.n_seqs = 0;
        sc_plan(K, S->img.rows.data(), I.count, I.sa_lo, max_walk, k_lo[t], R.n_segs, R.walked);
        off[t + 1] = off[t] + R.n_segs;
        occ_off[t + 1] = occ_off[t] + (R.n_segs ? R.count : 0);
    }
    const uint64_t n_segs = off[n_tasks], total = occ_off[n_tasks];
    phi_tab_t P; P.recs = S->img.phi.data(); P.dir = S->img.phi_dir.data();
    const loci_lift_t T = S->lift();
    unsigned long long n_phi = 0;
    std::vector<uint64_t> keys(total, ~0ull);           // exactly the walked total
    for (uint64_t g = 0; g < n_segs; ++g) {            // loci_walk_kernel, one lane per segment
        const uint64_t t = sc_task_of(off.data(), n_tasks, g);
        const moni_seqcount_res_t& R = sres[t];
        const uint32_t s = (uint32_t)(g - off[t]);
        const sc_seg_t G = sc_segment(K, S->T, S->img.rows.data(), S->img.cr.data(), S->img.recs.data(), R.sa_lo, R.count, toe[t], k_lo[t], R.n_segs, s);
        const uint64_t hi_rel = loci_seg_hi(S->img.rows.data(), R.sa_lo, R.count, k_lo[t], R.n_segs, s) - R.sa_lo;
        loci_seg_keys(K, P, T, G, t, hi_rel, lift, keys.data() + occ_off[t], n_phi);
    }
    {                                                  // the device sort looks at the bits below loci_key_bits alone: nothing may be set above them
        const uint32_t bits = loci_key_bits(n_tasks);
        for (uint64_t i = 0; i < total; ++i) if (bits < 64 && (keys[i] >> bits)) { fprintf(stderr, "loci_sim: key %llu has bits above %u\n", (unsigned long long)i, bits); keys[i] = 0; }
    }
    std::sort(keys.begin(), keys.end());
    std::vector<uint64_t> idx(total + 1, 0);           // loci_head_kernel and the scan of its flags
    for (uint64_t i = 0; i < total; ++i) idx[i + 1] = idx[i] + (loci_is_head(keys.data(), i) ? 1 : 0);
    const uint64_t n_loci = idx[total];
    O.lpos.assign(n_loci, 0); O.lseq.assign(n_loci, 0); O.lseq_off.assign(n_loci, 0); O.support.assign(n_loci, 0);
    std::vector<uint64_t> head(n_loci + 1, 0);
    for (uint64_t i = 0; i < total; ++i) {             // loci_emit_kernel
        if (!loci_is_head(keys.data(), i)) continue;
        const uint64_t j = idx[i], p = keys[i] & LOCI_POS_MASK;
        const uint32_t sid = seq_of(S->img.seq_starts.data(), K.n_seq, p);
        O.lpos[j] = p; O.lseq[j] = sid; O.lseq_off[j] = p - S->img.seq_starts[sid]; head[j] = i;
    }
    head[n_loci] = total;
    O.res.assign(n_tasks, moni_loci_res_t());
    for (uint64_t j = 0; j < n_loci; ++j) O.support[j] = head[j + 1] - head[j];          // loci_finish_kernel
    for (uint64_t t = 0; t < n_tasks; ++t) {
        const moni_seqcount_res_t& I = sres[t];
        moni_loci_res_t& R = O.res[t];
        R.count = I.count; R.sa_lo = I.sa_lo; R.matched = I.matched; R.walked = I.walked; R.n_segs = I.n_segs; R.reserved = 0;
        R.loci_off = total ? idx[occ_off[t]] : 0;
        R.n_loci = total ? idx[occ_off[t + 1]] - R.loci_off : 0;
    }
    O.counters[0] = N.steps; O.counters[1] = N.rows; O.counters[2] = n_phi; O.counters[3] = N.general;
    O.n_segs = n_segs; O.total = total;
}

// what loci_key meets at a text position: 1 the sequence moved past the directory entry's (the run is searched), 2 the directory's hint run had to be
// walked forward, 4 the position lies in the last directory block of the text, 8 the run found is an insertion, 16 the run in front of it is a deletion
__attribute__((unused)) static uint32_t key_shape(const LociSim* S, uint64_t pos) {
    const loci_lift_t T = S->lift();
    const uint64_t b = pos >> MONI_PDIR_SHIFT;
    const uint64_t e = T.pdir[b];
    uint32_t sid = (uint32_t)e, shape = 0;
    while (sid + 1 < T.n_seq && pos >= T.seqs[sid + 1].start) { ++sid; shape |= 1u; }
    const moni_lift_seq_t L = T.seqs[sid];
    const uint64_t start = pos - L.start;
    uint64_t x;
    const uint32_t k = L.run_off + lift_find(T.runs + L.run_off, L.n_runs, start, x);
    if (!(shape & 1u) && k != (uint32_t)(e >> 32)) shape |= 2u;
    if (b == (T.n_text >> MONI_PDIR_SHIFT)) shape |= 4u;
    if (T.runs[k].flags & MONI_LIFT_INS) shape |= 8u;
    if (k > L.run_off && (T.runs[k - 1].flags & MONI_LIFT_DEL) && start == T.runs[k].hap) shape |= 16u;
    return shape;
}

#ifndef LOCI_SIM_MAIN

static LociOut g_out;          // the last run's results (the tests are single-threaded)

extern "C" {
void* locisim_create(const moni_flat_index_t* f) { return sim_create(f); }
void locisim_destroy(void* s) { delete (LociSim*)s; }
// res[n_reads * strands]; sizes: loci, segments, walked total; counters[4].  The arrays wait for locisim_fetch.
void locisim_run(void* s, const uint8_t* seq, const uint64_t* offs, uint64_t n_reads, uint32_t strands, uint32_t lift, uint64_t max_walk, moni_loci_res_t* res, uint64_t* sizes,
                 uint64_t* counters) {
    sim_run((LociSim*)s, seq, offs, n_reads, strands, lift, max_walk, g_out);
    if (!g_out.res.empty()) memcpy(res, g_out.res.data(), g_out.res.size() * sizeof(moni_loci_res_t));
    sizes[0] = g_out.lpos.size(); sizes[1] = g_out.n_segs; sizes[2] = g_out.total;
    memcpy(counters, g_out.counters, sizeof(g_out.counters));
}
void locisim_fetch(uint64_t* lpos, uint32_t* lseq, uint64_t* lseq_off, uint64_t* support) {
    const size_t n = g_out.lpos.size();
    if (!n) return;
    memcpy(lpos, g_out.lpos.data(), n * 8); memcpy(lseq, g_out.lseq.data(), n * 4); memcpy(lseq_off, g_out.lseq_off.data(), n * 8); memcpy(support, g_out.support.data(), n * 8);
}
uint64_t locisim_key(void* s, uint64_t pos, uint32_t lift) { const loci_lift_t T = ((LociSim*)s)->lift(); return loci_key(T, pos, lift); }
uint32_t locisim_key_shape(void* s, uint64_t pos) { return key_shape((LociSim*)s, pos); }
}  // extern "C"

#else

// in:  10 u64 (n, r, w, n_seq, has_lcp, n_reads, strands, max_walk, lift, has_lifts), F[256], starts[r + 1], ssa[r], esa[r], thr[r], slcp[r] if has_lcp,
//      seq_starts[n_seq + 1], offs[n_reads + 1], and if has_lifts second[n_seq], len[n_seq], ins_off[n_seq + 1], ins[], del_off[n_seq + 1], del[] (u64 each),
//      then heads[r] and the patterns' bytes
// out: res[n_tasks] (48 bytes each), lpos[n_loci], lseq_off[n_loci], support[n_loci] (u64 each), lseq[n_loci] as u64, counters[4], segments, walked total, n_loci
template <class Tp>
static bool rd(FILE* f, std::vector<Tp>& v, size_t n) { v.resize(n); return !n || fread(v.data(), sizeof(Tp), n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint64_t> h, F, starts, ssa, esa, thr, slcp, seq_starts, offs, second, len, ins_off, ins, del_off, del;
    std::vector<uint8_t> heads, seq;
    bool ok = rd(f, h, 10);
    if (ok) {
        const uint64_t r = h[1], ns = h[3];
        ok = rd(f, F, 256) && rd(f, starts, r + 1) && rd(f, ssa, r) && rd(f, esa, r) && rd(f, thr, r) && (!h[4] || rd(f, slcp, r)) && rd(f, seq_starts, ns + 1) && rd(f, offs, h[5] + 1);
        if (ok && h[9]) ok = rd(f, second, ns) && rd(f, len, ns) && rd(f, ins_off, ns + 1) && rd(f, ins, ins_off.back()) && rd(f, del_off, ns + 1) && rd(f, del, del_off.back());
        ok = ok && rd(f, heads, r) && rd(f, seq, offs.empty() ? 0 : offs.back());
    }
    fclose(f);
    if (!ok) { fprintf(stderr, "loci_sim: short input\n"); return 2; }
    moni_flat_index_t fi;
    memset(&fi, 0, sizeof fi);
    fi.n = h[0]; fi.r = h[1]; fi.w = h[2]; fi.n_seq = h[3];
    fi.F = F.data(); fi.heads = heads.data(); fi.starts = starts.data(); fi.ssa = ssa.data(); fi.esa = esa.data(); fi.thr = thr.data();
    fi.slcp = h[4] ? slcp.data() : nullptr; fi.seq_starts = seq_starts.data();
    ins.resize(ins.size() + 1); del.resize(del.size() + 1);          // (never empty: the pointers are not null)
    if (h[9]) { fi.lift_second = second.data(); fi.lift_len = len.data(); fi.lift_ins_off = ins_off.data(); fi.lift_ins = ins.data(); fi.lift_del_off = del_off.data(); fi.lift_del = del.data(); }
    LociSim* S = sim_create(&fi);
    if (!S) return 3;
    seq.resize(seq.size() + 8, 0);
    LociOut O;
    sim_run(S, seq.data(), offs.data(), h[5], (uint32_t)h[6], (uint32_t)h[8], h[7], O);
    delete S;
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    auto wr = [&](const void* p, size_t sz, size_t n) { return !n || fwrite(p, sz, n, o) == n; };
    std::vector<uint64_t> sq64(O.lseq.begin(), O.lseq.end());
    const uint64_t tail[7] = {O.counters[0], O.counters[1], O.counters[2], O.counters[3], O.n_segs, O.total, (uint64_t)O.lpos.size()};
    ok = wr(O.res.data(), sizeof(moni_loci_res_t), O.res.size()) && wr(O.lpos.data(), 8, O.lpos.size()) && wr(O.lseq_off.data(), 8, O.lseq_off.size()) &&
         wr(O.support.data(), 8, O.support.size()) && wr(sq64.data(), 8, sq64.size()) && wr(tail, 8, 7);
    return fclose(o) == 0 && ok ? 0 : 2;
}

#endif
