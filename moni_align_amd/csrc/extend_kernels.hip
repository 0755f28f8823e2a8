// HIP kernels (gfx950) of extend mode: the reference's legacy `moni extend` (include/extender/extender_ksw2.hpp,
// include/extender/extend_reads_dispatcher.hpp:435-486).  Per read and strand: the single longest MEM, one ksw_extz2_sse extension
// to each side of it, one stitched CIGAR, a bowtie2-style MAPQ, one SAM line.
//
//   extend_rc_kernel      strand 1 of every read as extend_reads_dispatcher.hpp:460-461 makes it (see ext_complement)
//   extend_plan_kernel    one lane per (read, strand): find_longest_mem (extender_ksw2.hpp:261-296) over ms.query's pointers - the length
//                         loop of ms_len_kernel, the arg-max kept in registers, no length written to HBM - then a 32-byte plan record and
//                         up to two DP problems appended to a device-resident list (operands by position: DP_Q_READS / DP_T_TEXT)
//   extend_dp_kernel      extz_wave (extz_kernels.hip) over that list; nothing of it passes through the host
//   extend_finish_kernel  one wave per read, its two strands one after the other: score, threshold, ref_pos, CIGAR stitch, MD / NM
//                         (write_MD_core), MAPQ, line text into the record's staging slot; a record that is not written has length 0
// and the scan + gather_lines_kernel of the align stage put the lines of a chunk in read order.
//
// Deviations from the reference, both deliberate:
//   (1) left target with mem_pos <= ext_len: the reference expands ext_len - mem_pos bytes from position 0 (extender_ksw2.hpp:343-346), which
//       is not the text in front of the MEM and lets ref_pos run below zero; here the target is text [0, mem_pos) reversed.
//   (2) the @HD line is written with tabs (moni_sam_header), not with the blanks of extender_ksw2.hpp:741.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define EXT_MAX_READ DP_MAX_QLEN      // extz_wave keeps the query in LDS
#define EXT_MAX_TLEN 512              // extz_kernel<8>: 8 x 64 target rows
#define EXT_MAX_CIG 256               // operations of a stitched CIGAR
#define EXT_HEAD 1536                 // bytes of a line between the read's name and SEQ
#define EXT_TAIL 2560                 // bytes of a line behind QUAL
#define EXT_TAGS 48                   // ... of which "\tAS:i:", "\tNM:i:", "\tMD:Z:" and the two numbers
#define EXT_WIN (EXT_MAX_READ + 2 * EXT_MAX_TLEN)
#define EXT_NONE 0xFFFFFFFFu
// cursors of a chunk (unsigned long long each)
enum { EXC_TASKS = 0, EXC_DIR, EXC_CIG, EXC_ERR, EXC_RECORDS, EXC_EXTENDED, EXC_CELLS, EXC_BYTES, EXC_N };

// complement() of include/common/common.hpp:556-571, which extend_reads_dispatcher.hpp:460-461 applies to make strand 1: upper-case
// A / C / G / T only.  The library's strand-1 table (kpbseq.h:120-137, moni_tables_t::compl_tab) also maps a / c / g / t to T / G / C / A,
// so the two disagree on four of the 256 byte values and extend mode carries its own: this function, and the copy of the index tables
// with it as compl_tab that pack_kernel is given for this mode's matching statistics.
__host__ __device__ __forceinline__ uint8_t ext_complement(uint8_t b) { return b == 'A' ? 'T' : b == 'T' ? 'A' : b == 'G' ? 'C' : b == 'C' ? 'G' : b; }

struct alignas(32) ext_plan_t {       // find_longest_mem's result and where the two extensions are in the task list
    uint64_t mem_pos;
    uint32_t len, idx, L;
    uint32_t task_l, task_r;          // EXT_NONE: that side is empty (skipped, score 0)
    uint32_t dead;                    // a side has a query but no target (ksw2's untouched result, mqe = KSW_NEG_INF): no record
};

struct ext_args_t {
    moni_consts_t K;
    const uint8_t* text; const uint64_t* pat; const uint64_t* offs; const moni_u64x2* blk; const uint64_t* ptr;
    const uint8_t* seq2;              // the reads, then their strand-1 forms (same offsets + total_len)
    uint64_t total_len, read_lo, n_reads;      // this chunk: reads [read_lo, read_lo + n_reads)
    uint32_t min_len, ext_len; int32_t smatch;
    ext_plan_t* plans; moni_dp_task_t* tasks; uint64_t* dir_off; uint64_t* cig_off; unsigned long long* cur;
    uint64_t task_cap, dir_cap, cig_cap;
    // finish
    const moni_dp_result_t* res; const uint32_t* cig;
    const int32_t* min_score_of_len;  // (int32)(20 + 8 * log(L)) by libm on the host, extender_ksw2.hpp:222
    const uint64_t* seq_starts; const uint8_t* snames; const uint32_t* sname_off; uint32_t n_seq;
    const uint8_t* rnames; const uint64_t* rname_off; const uint8_t* quals;
    uint8_t* lines; uint64_t slot;    // staging: record g of the chunk owns lines[g * slot, (g + 1) * slot), slot a multiple of 8
    uint64_t* len; uint64_t* off;     // per record: bytes of its line (0: none), its slot in 8-byte words (gather_lines_kernel)
};

__global__ void __launch_bounds__(256) extend_rc_kernel(const uint8_t* __restrict__ seq, const uint64_t* __restrict__ offs, uint64_t n_reads, uint8_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const uint64_t r = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (r >= n_reads) return;
    const uint64_t off = offs[r];
    const uint32_t m = (uint32_t)(offs[r + 1] - off);
    for (uint32_t k = lane; k < m; k += 64) out[off + k] = ext_complement(seq[off + m - 1 - k]);
}

__device__ __forceinline__ uint32_t ext_wave_scan(uint32_t v, uint32_t& total) {      // exclusive prefix sum over the wave
    const int lane = threadIdx.x & 63;
    uint32_t inc = v;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t x = (uint32_t)__shfl_up((int)inc, o); if (lane >= o) inc += x; }
    total = (uint32_t)__shfl((int)inc, 63);
    return inc - v;
}
__device__ __forceinline__ unsigned long long ext_bcast64(unsigned long long v, int src) {
    return ((unsigned long long)(uint32_t)__shfl((int)(v >> 32), src) << 32) | (uint32_t)__shfl((int)(v & 0xFFFFFFFFull), src);
}

__global__ void __launch_bounds__(MS_BLOCK) extend_plan_kernel(const ext_args_t X) {
    const int lane = threadIdx.x & 63;
    const uint64_t g = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;      // record of the chunk: 2 * (read - read_lo) + strand
    const bool live = g < 2 * X.n_reads;
    ext_plan_t P;
    P.mem_pos = 0; P.len = 0; P.idx = 0; P.L = 0; P.task_l = EXT_NONE; P.task_r = EXT_NONE; P.dead = 0;
    moni_dp_task_t tl, tr;
    uint32_t n_t = 0, n_dir = 0, n_cig = 0;
    bool has_l = false, has_r = false;
    unsigned long long cells = 0;
    if (live) {
        const uint64_t read = X.read_lo + (g >> 1), task = 2 * X.read_lo + g;
        const uint32_t strand = (uint32_t)g & 1u;
        const uint64_t pb = ws_pat_base(X.blk, task), qb = ws_ptr_base(X.blk, task);
        const uint64_t off = X.offs[read];
        const uint32_t m = (uint32_t)(X.offs[read + 1] - off);
        const uint64_t n = X.K.n_text;
        P.L = m;
        // find_longest_mem: the first position whose length is strictly greater than the best so far, and the n_Ns rule as written
        uint64_t l = 0, prev_pos_plus_one = n + 1, n_Ns = 0, mem_pos = 0;
        uint32_t mem_len = 0, mem_idx = 0;
        pat_cache_t pc; pc.w = 0xFFFFFFFFu; pc.word = 0;
        text_cache_t tc; tc.w = ~0ull; tc.word = 0;
        for (uint32_t i = 0; i < m; ++i) {
            const uint64_t pos = X.ptr[qb + (uint64_t)(m - 1 - i) * 64u];
            while (pos != prev_pos_plus_one && (i + l) < m && (pos + l) < n) {
                const uint8_t b = pat_byte(X.pat, pb, m, (uint32_t)(i + l), pc);
                if (b != text_byte(X.text, pos + l, tc)) break;
                n_Ns = b == 'N' ? n_Ns + 1 : 0;
                ++l;
            }
            if (l > mem_len && n_Ns < l) { mem_len = (uint32_t)l; mem_pos = pos; mem_idx = i; }
            l = (l == 0 ? 0 : (l - 1));
            prev_pos_plus_one = pos + 1;
        }
        P.mem_pos = mem_pos; P.len = mem_len; P.idx = mem_idx;
        if (mem_len > 0 && mem_len >= X.min_len && m > EXT_MAX_READ) P.dead = 1;          // (the host refuses such a batch before it gets here)
        else if (mem_len > 0 && mem_len >= X.min_len) {
            const uint64_t base = (strand ? X.total_len : 0) + off, E = X.ext_len;
            const uint32_t lcs = mem_idx, rcs = m - mem_idx - mem_len;
            const int flag = DP_EZ_EXTZ_ONLY | DP_EZ_RIGHT;
            if (lcs > 0) {          // query: read [0, idx) reversed; target: the text in front of the MEM, reversed
                const uint64_t tlen = mem_pos > E ? E : mem_pos;
                if (!tlen) P.dead = 1;
                else {
                    has_l = true;
                    tl.q_off = base + lcs - 1; tl.t_off = mem_pos - 1; tl.qlen = (int32_t)lcs; tl.tlen = (int32_t)tlen; tl.flag = flag;
                    tl.reserved = DP_Q_READS | DP_Q_REV | DP_T_TEXT | DP_T_REV;
                }
            }
            if (rcs > 0) {
                const uint64_t rc_occ = mem_pos + mem_len;
                const uint64_t tlen = rc_occ + E < n ? E : n - rc_occ;
                if (!tlen) P.dead = 1;
                else {
                    has_r = true;
                    tr.q_off = base + mem_idx + mem_len; tr.t_off = rc_occ; tr.qlen = (int32_t)rcs; tr.tlen = (int32_t)tlen; tr.flag = flag;
                    tr.reserved = DP_Q_READS | DP_T_TEXT;
                }
            }
            if (P.dead) has_l = has_r = false;
            if (has_l) { ++n_t; n_dir += (uint32_t)(tl.qlen + tl.tlen - 1) * (uint32_t)tl.tlen; n_cig += (uint32_t)(tl.qlen + tl.tlen + 2); cells += (unsigned long long)tl.qlen * tl.tlen; }
            if (has_r) { ++n_t; n_dir += (uint32_t)(tr.qlen + tr.tlen - 1) * (uint32_t)tr.tlen; n_cig += (uint32_t)(tr.qlen + tr.tlen + 2); cells += (unsigned long long)tr.qlen * tr.tlen; }
        }
    }
    // the wave's problems take consecutive places in the list: one bump of the three cursors per wave, checked against the capacities
    uint32_t tot_t, tot_d, tot_c;
    const uint32_t at_t = ext_wave_scan(n_t, tot_t), at_d = ext_wave_scan(n_dir, tot_d), at_c = ext_wave_scan(n_cig, tot_c);
    unsigned long long b_t = 0, b_d = 0, b_c = 0;
    if (lane == 0 && tot_t) { b_t = atomicAdd(&X.cur[EXC_TASKS], (unsigned long long)tot_t); b_d = atomicAdd(&X.cur[EXC_DIR], (unsigned long long)tot_d); b_c = atomicAdd(&X.cur[EXC_CIG], (unsigned long long)tot_c); }
    b_t = ext_bcast64(b_t, 0); b_d = ext_bcast64(b_d, 0); b_c = ext_bcast64(b_c, 0);
    const bool fits = b_t + tot_t <= X.task_cap && b_d + tot_d <= X.dir_cap && b_c + tot_c <= X.cig_cap;
    if (!fits) {          // never with the capacities the host derives from the read lengths; were they wrong the batch fails, nothing is written past them
        if (lane == 0) atomicMax(&X.cur[EXC_ERR], 1ull);
        has_l = has_r = false; P.dead = 1;
    }
    if (live) {
        uint64_t t = b_t + at_t, d = b_d + at_d, cg = b_c + at_c;
        if (has_l) {
            P.task_l = (uint32_t)t; X.tasks[t] = tl; X.dir_off[t] = d; X.cig_off[t] = cg;
            ++t; d += (uint64_t)(tl.qlen + tl.tlen - 1) * tl.tlen; cg += (uint64_t)(tl.qlen + tl.tlen + 2);
        }
        if (has_r) { P.task_r = (uint32_t)t; X.tasks[t] = tr; X.dir_off[t] = d; X.cig_off[t] = cg; }
        X.plans[g] = P;
    }
    wave_add(cells, &X.cur[EXC_CELLS]);
}

// extz_wave over the device-resident list: persistent one-wave blocks, problem t of the list for t = block, block + grid, ...
template <int NCH>
__global__ void __launch_bounds__(64) extend_dp_kernel(const dp_launch_t P, const unsigned long long* __restrict__ n_tasks, uint64_t task_cap) {
    __shared__ uint8_t qs[DP_MAX_QLEN];
    const uint64_t n = *n_tasks < task_cap ? *n_tasks : task_cap;
    for (uint64_t t = blockIdx.x; t < n; t += gridDim.x) {
        const moni_dp_task_t task = P.tasks[t];
        moni_dp_result_t R;
        extz_wave<NCH>(P, task, qs, P.dirs + P.dir_off[t], P.cig_tmp + P.cig_off[t], R);
        if (threadIdx.x == 0) P.results[t] = R;
    }
}

// bowtie2's table for an alignment without a valid second best (extender_ksw2.hpp:806-807)
__constant__ uint8_t ext_unp_nosec[11] = {43, 42, 41, 36, 32, 27, 20, 11, 4, 1, 0};

struct ext_fin_t {
    uint8_t rd[EXT_MAX_READ];         // the strand's sequence, nt4
    uint8_t rf[EXT_WIN];              // text [ref_pos, ref_pos + ref_len), nt4
    uint32_t cig[EXT_MAX_CIG];
    uint8_t head[EXT_HEAD];
    uint8_t tail[EXT_TAIL];
};

struct ext_buf_t {          // bounded text: a byte past the capacity is dropped and remembered
    uint8_t* p; uint32_t cap, n; bool over;
    __device__ __forceinline__ void ch(uint8_t c) { if (n < cap) p[n++] = c; else over = true; }
    __device__ __forceinline__ void lit(const char* s) { while (*s) ch((uint8_t)*s++); }
    __device__ __forceinline__ void num(uint32_t v) {
        uint8_t d[10]; int k = 0;
        do { d[k++] = (uint8_t)('0' + v % 10u); v /= 10u; } while (v);
        while (k) ch(d[--k]);
    }
    __device__ __forceinline__ void inum(int32_t v) { if (v < 0) { ch('-'); num(0u - (uint32_t)v); } else num((uint32_t)v); }
};

__global__ void __launch_bounds__(64) extend_finish_kernel(const ext_args_t X) {
    __shared__ ext_fin_t S;
    __shared__ uint32_t sh[8];
    const int lane = threadIdx.x;
    for (uint64_t r_in = blockIdx.x; r_in < X.n_reads; r_in += gridDim.x) {
        const uint64_t read = X.read_lo + r_in;
        const uint64_t off = X.offs[read];
        const uint32_t m = (uint32_t)(X.offs[read + 1] - off);
        const uint64_t n0 = X.rname_off[read], n1 = X.rname_off[read + 1];
        bool any = false;
        for (uint32_t strand = 0; strand < 2; ++strand) {
            const uint64_t g = 2 * r_in + strand;
            const ext_plan_t P = X.plans[g];
            uint64_t out_len = 0;
            const bool cand = P.len > 0 && P.len >= X.min_len && !P.dead && m <= EXT_MAX_READ;
            moni_dp_result_t Rl, Rr;
            Rl.mqe = 0; Rl.mqe_t = -1; Rl.n_cigar = 0; Rr = Rl;
            uint64_t cl = 0, cr = 0;
            if (cand && P.task_l != EXT_NONE) { Rl = X.res[P.task_l]; cl = X.cig_off[P.task_l]; }
            if (cand && P.task_r != EXT_NONE) { Rr = X.res[P.task_r]; cr = X.cig_off[P.task_r]; }
            // (each mqe is at least KSW_NEG_INF = -2^30: the sum stays inside int32)
            const int32_t score = (int32_t)P.len * X.smatch + Rl.mqe + Rr.mqe;
            const int32_t min_score = X.min_score_of_len[m];
            if (cand && score > min_score) {
                const uint32_t span_l = P.task_l != EXT_NONE ? (uint32_t)(Rl.mqe_t + 1) : 0u, span_r = P.task_r != EXT_NONE ? (uint32_t)(Rr.mqe_t + 1) : 0u;
                const uint64_t ref_pos = P.mem_pos - span_l;
                const uint32_t ref_len = span_l + P.len + span_r;
                const uint8_t* __restrict__ sq = X.seq2 + (strand ? X.total_len : 0) + off;
                __syncthreads();
                for (uint32_t k = lane; k < m; k += 64) S.rd[k] = (uint8_t)dp_nt4(sq[k]);
                for (uint32_t k = lane; k < ref_len && k < EXT_WIN; k += 64) { const uint64_t a = ref_pos + k; S.rf[k] = (uint8_t)dp_nt4(a < X.K.n_text ? X.text[a] : 0u); }
                __syncthreads();
                if (lane == 0) {
                    bool over = ref_len > EXT_WIN;
                    // ---- the CIGAR: the left one backwards, len M, the right one; M merges into an M beside it (extender_ksw2.hpp:463-490) ----
                    uint32_t nc = 0;
                    if ((uint64_t)Rl.n_cigar + Rr.n_cigar + 1 > EXT_MAX_CIG) over = true;
                    else {
                        for (uint32_t j = 0; j < Rl.n_cigar; ++j) S.cig[nc++] = X.cig[cl + Rl.n_cigar - 1 - j];
                        if (nc > 0 && (S.cig[nc - 1] & 0xfu) == 0) S.cig[nc - 1] += P.len << 4; else S.cig[nc++] = P.len << 4;
                        if (Rr.n_cigar > 0) { const uint32_t c0 = X.cig[cr]; if ((c0 & 0xfu) == 0) S.cig[nc - 1] += c0; else S.cig[nc++] = c0; }
                        for (uint32_t j = 1; j < Rr.n_cigar; ++j) S.cig[nc++] = X.cig[cr + j];
                    }
                    // ---- RNAME, POS: seqidx::index (seqidx.hpp:149-154) of ref_pos in the concatenation, no lift-over ----
                    uint32_t lo = 0, hi = X.n_seq;          // the last sequence that starts at or before ref_pos
                    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (X.seq_starts[mid] <= ref_pos) lo = mid; else hi = mid; }
                    const uint32_t sid = lo;
                    // ---- MAPQ: compute_mapq with score2 = 0 (extender_ksw2.hpp:649-675), the operations in the host's order, none contracted ----
                    const int32_t max_score = (int32_t)m * X.smatch, best = max_score - score;
                    const double binf = __dadd_rn(__dmul_rn((double)best, __ddiv_rn(10.0, (double)(max_score - min_score))), 0.5);
                    uint32_t bin = binf > 0.0 ? (uint32_t)binf : 0u;
                    if (bin > 10u) bin = 10u;
                    const uint32_t mapq = best == max_score ? 44u : ext_unp_nosec[bin];
                    ext_buf_t H; H.p = S.head; H.cap = EXT_HEAD; H.n = 0; H.over = false;
                    H.lit(strand ? "\t16\t" : "\t0\t");
                    for (uint32_t k = X.sname_off[sid]; k < X.sname_off[sid + 1]; ++k) H.ch(X.snames[k]);
                    H.ch('\t'); H.num((uint32_t)(ref_pos - X.seq_starts[sid] + 1)); H.ch('\t'); H.num(mapq); H.ch('\t');
                    for (uint32_t k = 0; k < nc; ++k) { H.num(S.cig[k] >> 4); const uint32_t op = S.cig[k] & 0xfu; H.ch(op == 0 ? 'M' : op == 1 ? 'I' : 'D'); }
                    H.lit("\t*\t0\t0\t");
                    // ---- MD / NM: write_MD_core (extender_ksw2.hpp:526-576) over the window and the strand's sequence ----
                    // NM precedes MD in the line and is known only after the walk: MD is written EXT_TAGS bytes into the buffer (the tags in front of it
                    // take at most 17 + 16 + 6) and moved down behind them afterwards
                    uint32_t q_off = 0, t_off = 0, l_md = 0, nm = 0;
                    ext_buf_t M; M.p = S.tail + EXT_TAGS; M.cap = EXT_TAIL - EXT_TAGS - 1; M.n = 0; M.over = false;
                    const char* bases = "ACGTN";
                    for (uint32_t k = 0; k < nc; ++k) {
                        const uint32_t op = S.cig[k] & 0xfu, len = S.cig[k] >> 4;
                        if (op == 0) {
                            for (uint32_t j = 0; j < len; ++j) {
                                const uint32_t qa = q_off + j < EXT_MAX_READ ? q_off + j : EXT_MAX_READ - 1, ta = t_off + j < EXT_WIN ? t_off + j : EXT_WIN - 1;
                                if (S.rd[qa] != S.rf[ta]) { M.num(l_md); M.ch((uint8_t)bases[S.rf[ta] > 4 ? 4 : S.rf[ta]]); l_md = 0; ++nm; }
                                else ++l_md;
                            }
                            q_off += len; t_off += len;
                        } else if (op == 1) { q_off += len; nm += len; }
                        else if (op == 2) {
                            M.num(l_md); M.ch('^');
                            for (uint32_t j = 0; j < len; ++j) { const uint32_t ta = t_off + j < EXT_WIN ? t_off + j : EXT_WIN - 1; M.ch((uint8_t)bases[S.rf[ta] > 4 ? 4 : S.rf[ta]]); }
                            l_md = 0; t_off += len; nm += len;
                        }
                    }
                    if (l_md > 0) M.num(l_md);
                    ext_buf_t T; T.p = S.tail; T.cap = EXT_TAGS; T.n = 0; T.over = false;
                    T.lit("\tAS:i:"); T.inum(score); T.lit("\tNM:i:"); T.num(nm); T.lit("\tMD:Z:");
                    over = over || H.over || M.over || T.over;
                    if (!over) {
                        for (uint32_t k = 0; k < M.n; ++k) S.tail[T.n + k] = S.tail[EXT_TAGS + k];          // (downwards: a forward copy)
                        S.tail[T.n + M.n] = '\n';
                    }
                    sh[0] = over ? 1u : 0u; sh[1] = H.n; sh[2] = T.n + M.n + 1;
                }
                __syncthreads();
                const uint32_t over = sh[0], hn = sh[1], tn = sh[2];
                const uint32_t nl = (uint32_t)(n1 - n0);
                const uint64_t total = (uint64_t)nl + hn + m + 1 + (X.quals ? m : 1u) + tn;
                if (over || total > X.slot) { if (lane == 0) atomicMax(&X.cur[EXC_ERR], 2ull); }
                else {
                    uint8_t* __restrict__ o = X.lines + g * X.slot;
                    for (uint32_t k = lane; k < nl; k += 64) o[k] = X.rnames[n0 + k];
                    o += nl;
                    for (uint32_t k = lane; k < hn; k += 64) o[k] = S.head[k];
                    o += hn;
                    for (uint32_t k = lane; k < m; k += 64) o[k] = sq[k];
                    o += m;
                    if (lane == 0) o[0] = '\t';
                    o += 1;
                    if (X.quals) { for (uint32_t k = lane; k < m; k += 64) o[k] = X.quals[strand ? off + m - 1 - k : off + k]; o += m; }
                    else { if (lane == 0) o[0] = '*'; o += 1; }
                    for (uint32_t k = lane; k < tn; k += 64) o[k] = S.tail[k];
                    out_len = total;
                    any = true;
                }
            } else if (P.len > 0 && P.len >= X.min_len && m > EXT_MAX_READ) { if (lane == 0) atomicMax(&X.cur[EXC_ERR], 2ull); }
            if (lane == 0) {
                X.len[g] = out_len; X.off[g] = g * (X.slot >> 3);
                if (out_len) { atomicAdd(&X.cur[EXC_RECORDS], 1ull); atomicAdd(&X.cur[EXC_BYTES], (unsigned long long)out_len); }
            }
        }
        if (lane == 0 && any) atomicAdd(&X.cur[EXC_EXTENDED], 1ull);
    }
}
