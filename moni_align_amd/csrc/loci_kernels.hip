// HIP kernels (gfx950) of the loci query; the per-lane logic is in loci_core.h.  Included from moni_hip.hip after seqcount_kernels.hip
// (seqcount_plan_kernel, SC_MINW, MS_BLOCK, wave_add).
//
// Mapping: the search is count_kernel's and the segments are seqcount_plan_kernel's.  loci_plan_kernel, one lane per task, gives every walked task
// count slots of the key buffer.  loci_walk_kernel has one LANE per SEGMENT, as seqcount_walk_kernel has; where that kernel adds into a table, this
// one lifts every position (directory entry, sequence record, one or two runs: three more dependent loads behind the three of the phi step) and
// stores the key at the slot of the position's rank - a plain 8-byte vector store, no atomic.  rocPRIM sorts the buffer; loci_head_kernel, the scan
// of its flags, loci_emit_kernel and loci_finish_kernel fold it: one lane per sorted key, per locus and per task.
#include "loci_core.h"

// res: seqcount_plan_kernel's; walk_cnt: n_tasks + 1 entries for the scan.  Thread n_tasks closes it, and puts the number of segments (seg_off: their
// scan) behind where the scan of walk_cnt will put the number of walked occurrences: the host fetches both with one copy.
__global__ void __launch_bounds__(MS_BLOCK)
loci_plan_kernel(uint64_t n_tasks, const moni_seqcount_res_t* __restrict__ res, const uint64_t* __restrict__ seg_off, uint64_t* __restrict__ walk_cnt,
                 uint64_t* __restrict__ occ_off) {
    const uint64_t t = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (t < n_tasks) walk_cnt[t] = res[t].n_segs ? res[t].count : 0;          // (n_segs > 0: walked and count > 0)
    else if (t == n_tasks) { walk_cnt[t] = 0; occ_off[n_tasks + 1] = seg_off[n_tasks]; }
}

// off: the exclusive scan of the segment counts, total = off[n_tasks] > 0; occ_off: the exclusive scan of the walked counts; keys: occ_off[n_tasks] slots.
// Grid-stride over the segments, as in seqcount_walk_kernel.
__global__ void __launch_bounds__(MS_BLOCK, SC_MINW)
loci_walk_kernel(const moni_consts_t K, const phi_tab_t P, const loci_lift_t T, const moni_row_t* __restrict__ rows, const uint32_t* __restrict__ cr,
                 const moni_rec_t* __restrict__ recs, uint64_t n_tasks, uint64_t total, uint32_t lift, const moni_seqcount_res_t* __restrict__ res,
                 const uint64_t* __restrict__ toe, const uint32_t* __restrict__ k_lo, const uint64_t* __restrict__ off, const uint64_t* __restrict__ occ_off,
                 uint64_t* __restrict__ keys, unsigned long long* __restrict__ counters) {
    __shared__ sc_tabs_t S;
    if (threadIdx.x < MONI_MAX_SIGMA) { S.rec_base[threadIdx.x] = K.rec_base[threadIdx.x]; S.hot_slot[threadIdx.x] = K.hot_slot[threadIdx.x]; }
    __syncthreads();
    unsigned long long n_phi = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x; g < total; g += (uint64_t)gridDim.x * MS_BLOCK) {
        const uint64_t t = sc_task_of(off, n_tasks, g);
        const moni_seqcount_res_t R = res[t];
        const uint32_t kl = k_lo[t], s = (uint32_t)(g - off[t]);
        const sc_seg_t G = sc_segment(K, S, rows, cr, recs, R.sa_lo, R.count, toe[t], kl, R.n_segs, s);
        const uint64_t hi_rel = loci_seg_hi(rows, R.sa_lo, R.count, kl, R.n_segs, s) - R.sa_lo;
        loci_seg_keys(K, P, T, G, t, hi_rel, lift, keys + occ_off[t], n_phi);
    }
    wave_add(n_phi, &counters[2]);
}

// flag: n + 1 entries for the scan (thread n closes it)
__global__ void __launch_bounds__(MS_BLOCK)
loci_head_kernel(const uint64_t* __restrict__ sorted, uint64_t n, uint64_t* __restrict__ flag) {
    const uint64_t i = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i < n) flag[i] = loci_is_head(sorted, i) ? 1 : 0;
    else if (i == n) flag[i] = 0;
}

// idx: the exclusive scan of the flags (n + 1 entries, idx[n] = the number of loci); head: idx[n] + 1 entries (thread n closes it with n)
__global__ void __launch_bounds__(MS_BLOCK)
loci_emit_kernel(const uint64_t* __restrict__ sorted, uint64_t n, const uint64_t* __restrict__ idx, const uint64_t* __restrict__ seq_starts, uint32_t n_seq,
                 uint64_t* __restrict__ lpos, uint32_t* __restrict__ lseq, uint64_t* __restrict__ lseq_off, uint64_t* __restrict__ head) {
    const uint64_t i = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i < n) {
        if (!loci_is_head(sorted, i)) return;
        const uint64_t j = idx[i], p = sorted[i] & LOCI_POS_MASK;
        const uint32_t sid = seq_of(seq_starts, n_seq, p);
        lpos[j] = p; lseq[j] = sid; lseq_off[j] = p - seq_starts[sid]; head[j] = i;
    } else if (i == n) head[idx[n]] = n;
}

// One lane per locus (its support) and per task (its record).  idx == nullptr: nothing was walked, every task has no locus.
__global__ void __launch_bounds__(MS_BLOCK)
loci_finish_kernel(uint64_t n_tasks, uint64_t n_loci, const moni_seqcount_res_t* __restrict__ res_in, const uint64_t* __restrict__ occ_off,
                   const uint64_t* __restrict__ idx, const uint64_t* __restrict__ head, uint64_t* __restrict__ support, moni_loci_res_t* __restrict__ res) {
    const uint64_t i = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i < n_loci) support[i] = head[i + 1] - head[i];
    if (i < n_tasks) {
        const moni_seqcount_res_t I = res_in[i];
        moni_loci_res_t R;
        R.count = I.count; R.sa_lo = I.sa_lo; R.matched = I.matched; R.walked = I.walked; R.n_segs = I.n_segs; R.reserved = 0;
        R.loci_off = idx ? idx[occ_off[i]] : 0;
        R.n_loci = idx ? idx[occ_off[i + 1]] - R.loci_off : 0;
        res[i] = R;
    }
}
