// HIP kernels (gfx950) of the exact-match queries, count and locate; the per-lane logic is in locate_core.h.  Included from moni_hip.hip after
// seed_kernels.hip (MS_BLOCK, load_tables, wave_add).
//
// Mapping: one LANE per (pattern, strand), as ms_lf_kernel has: every step is one or two dependent random 64-byte row fetches, so 64 patterns per
// wavefront keep 64 to 128 of them in flight.  The state is two (run, off) pairs, the toehold and one pattern word: 8 waves per SIMD.  A lane whose
// interval empties leaves the loop; its wavefront goes on until its longest survivor is through.  locate_walk_kernel has one lane per task as
// well: n_occ - 1 dependent phi steps each, the positions written at the task's offset of the scan.
#include "locate_core.h"

#define LOC_MINW 8          // waves per SIMD the register allocator must leave room for (DESIGN.md 7.5 has the figures)

// task t = pattern * strands + strand (strands 1 or 2); thread n_tasks closes cnt for the exclusive scan
__global__ void __launch_bounds__(MS_BLOCK, LOC_MINW)
count_kernel(const moni_consts_t K, const moni_tables_t* __restrict__ T, const moni_row_t* __restrict__ rows, const moni_frow_t* __restrict__ frows,
             const uint32_t* __restrict__ cr, const moni_rec_t* __restrict__ recs, const uint64_t* __restrict__ pat, const uint64_t* __restrict__ offs,
             const moni_u64x2* __restrict__ blk, uint64_t n_tasks, uint32_t strands, uint32_t max_occ, moni_locate_res_t* __restrict__ res,
             uint64_t* __restrict__ toe, uint64_t* __restrict__ cnt, unsigned long long* __restrict__ counters) {
    __shared__ lds_tables_t L;
    load_tables(L, T, K);
    const uint64_t t = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    loc_counts_t N; N.steps = N.rows = N.general = N.phi = 0;
    if (t < n_tasks) {
        moni_locate_res_t R;
        uint64_t th;
        loc_task(K, L, rows, frows, cr, recs, pat, offs, blk, strands == 2 ? t >> 1 : t, strands == 2 ? (uint32_t)t & 1u : 0u, max_occ, R, th, N);
        res[t] = R;
        toe[t] = th;
        cnt[t] = R.n_occ;
    } else if (t == n_tasks) cnt[t] = 0;
    wave_add(N.steps, &counters[0]);
    wave_add(N.rows, &counters[1]);
    wave_add(N.general, &counters[3]);
}

// off: the exclusive scan of the capped counts (n_tasks + 1 entries); pos / seq / seq_off hold off[n_tasks] entries
__global__ void __launch_bounds__(MS_BLOCK)
locate_walk_kernel(const moni_consts_t K, const phi_tab_t P, const uint64_t* __restrict__ seq_starts, uint64_t n_tasks, moni_locate_res_t* __restrict__ res,
                   const uint64_t* __restrict__ toe, const uint64_t* __restrict__ off, uint64_t* __restrict__ pos, uint32_t* __restrict__ seq,
                   uint64_t* __restrict__ seq_off, unsigned long long* __restrict__ counters) {
    const uint64_t t = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    loc_counts_t N; N.steps = N.rows = N.general = N.phi = 0;
    if (t < n_tasks) {
        const uint32_t n_occ = res[t].n_occ;
        const uint64_t o = off[t];
        res[t].occ_off = o;
        if (n_occ) loc_walk(K, P, seq_starts, toe[t], n_occ, pos + o, seq + o, seq_off + o, N);
    }
    wave_add(N.phi, &counters[2]);
}
