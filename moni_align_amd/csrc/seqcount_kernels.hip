// HIP kernels (gfx950) of the sequence-count query; the per-lane logic is in seqcount_core.h.  Included from moni_hip.hip after locate_kernels.hip
// (count_kernel, MS_BLOCK, wave_add).
//
// Mapping: the search is count_kernel's, one lane per (pattern, strand).  seqcount_plan_kernel, one lane per task, finds the runs of the interval's two
// ends; the exclusive scan of the segment counts numbers the segments of the batch.  seqcount_walk_kernel has one LANE per SEGMENT - the part of an
// interval inside one BWT run - so a pattern whose interval spans m runs is m lanes whose walks are as short as the runs, where locate_walk_kernel
// has one lane of count steps.  Every phi step is three dependent accesses (directory, keys, record), as in occ_kernel: latency-bound, so the kernel
// asks for 8 waves per SIMD and holds no more state than a position, a length and the running (sequence, count) pair.  The adds are 64-bit atomics
// without a return value into the task's row of the table in HBM.
#include "seqcount_core.h"

#define SC_MINW 8           // waves per SIMD the register allocator must leave room for (DESIGN.md 7.6 has the figures)

// res_in / toe: count_kernel's; seg_cnt: n_tasks + 1 entries for the scan (thread n_tasks closes it)
__global__ void __launch_bounds__(MS_BLOCK)
seqcount_plan_kernel(const moni_consts_t K, const moni_row_t* __restrict__ rows, uint64_t n_tasks, uint64_t max_walk, const moni_locate_res_t* __restrict__ res_in,
                     moni_seqcount_res_t* __restrict__ res, uint32_t* __restrict__ k_lo, uint64_t* __restrict__ seg_cnt) {
    const uint64_t t = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (t < n_tasks) {
        const moni_locate_res_t I = res_in[t];
        moni_seqcount_res_t R;
        R.count = I.count; R.sa_lo = I.sa_lo; R.matched = I.matched; R.n_seqs = 0;
        uint32_t kl;
        sc_plan(K, rows, I.count, I.sa_lo, max_walk, kl, R.n_segs, R.walked);
        res[t] = R;
        k_lo[t] = kl;
        seg_cnt[t] = R.n_segs;
    } else if (t == n_tasks) seg_cnt[t] = 0;
}

// off: the exclusive scan of the segment counts (n_tasks + 1 entries), total = off[n_tasks] > 0; counts: n_tasks rows of K.n_seq, zeroed.
// Grid-stride over the segments: the grid is capped, the segment index is 64-bit.
__global__ void __launch_bounds__(MS_BLOCK, SC_MINW)
seqcount_walk_kernel(const moni_consts_t K, const phi_tab_t P, const moni_row_t* __restrict__ rows, const uint32_t* __restrict__ cr, const moni_rec_t* __restrict__ recs,
                     const uint64_t* __restrict__ seq_starts, uint64_t n_tasks, uint64_t total, const moni_seqcount_res_t* __restrict__ res,
                     const uint64_t* __restrict__ toe, const uint32_t* __restrict__ k_lo, const uint64_t* __restrict__ off, unsigned long long* __restrict__ counts,
                     unsigned long long* __restrict__ counters) {
    __shared__ sc_tabs_t T;
    if (threadIdx.x < MONI_MAX_SIGMA) { T.rec_base[threadIdx.x] = K.rec_base[threadIdx.x]; T.hot_slot[threadIdx.x] = K.hot_slot[threadIdx.x]; }
    __syncthreads();
    unsigned long long n_phi = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x; g < total; g += (uint64_t)gridDim.x * MS_BLOCK) {
        const uint64_t t = sc_task_of(off, n_tasks, g);
        const moni_seqcount_res_t R = res[t];
        const sc_seg_t G = sc_segment(K, T, rows, cr, recs, R.sa_lo, R.count, toe[t], k_lo[t], R.n_segs, (uint32_t)(g - off[t]));
        unsigned long long* __restrict__ row = counts + t * K.n_seq;
        sc_seg_count(K, P, seq_starts, G, n_phi, [&](uint32_t sid, uint64_t v) { atomicAdd(row + sid, (unsigned long long)v); });
    }
    wave_add(n_phi, &counters[2]);
}

// n_seqs: the non-zero entries of a walked task's row
__global__ void __launch_bounds__(MS_BLOCK)
seqcount_finish_kernel(uint32_t n_seq, uint64_t n_tasks, const unsigned long long* __restrict__ counts, moni_seqcount_res_t* __restrict__ res) {
    const uint64_t t = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (t >= n_tasks || !res[t].n_segs) return;
    const unsigned long long* __restrict__ row = counts + t * n_seq;
    uint32_t k = 0;
    for (uint32_t s = 0; s < n_seq; ++s) k += row[s] != 0;
    res[t].n_seqs = k;
}
