// HIP kernels (gfx950) of the k-mismatch queries; the per-lane logic is in approx_core.h.  Included from moni_hip.hip after seqcount_kernels.hip
// (MS_BLOCK, load_tables, wave_add, loc_walk).
//
// Mapping: approx_exact_kernel is count_kernel with checkpoints, one lane per (pattern, strand).  approx_tree_kernel has one LANE per (task, chunk):
// the subtrees that leave the exact path inside a chunk of chunk_len places are one lane's depth-first walk.  Every step is one or two dependent
// random 64-byte row fetches, as in count_kernel: latency-bound, and the lanes of a wavefront diverge in depth.  Measured, the cut
// does not pay on the benchmark's reads: most of a task's tree hangs off the first dozen places, where the interval is still wide, so one piece
// carries it and the others leave their wavefronts mostly idle - the default chunk_len is one piece per task, and the parameter stays for patterns
// whose tree is spread out.  Level 0 and the active level live in registers; the (at most two) levels in between are parked in LDS as
// [level][word][lane], five 8-byte words each: 20 KB per block of 256 beside the 4 KB of tables.  The sums go to the task's record with 64-bit
// atomics without a return value, one per lane and distance at the end of the piece; a hit takes its slot with an atomicAdd on the task's kept
// counter.
#include "approx_core.h"

#define APX_MINW 4          // waves per SIMD the register allocator must leave room for: the tree walk (DESIGN.md 7.8 has the figures)
#define APX_EXACT_MINW 6    // ... the exact pass: count_kernel's loop and a checkpoint to pack (8 would spill)
#define APX_MAX_GRID (1u << 20)

// cnt: n_tasks + 1 entries for the scan (thread n_tasks closes it)
__global__ void __launch_bounds__(MS_BLOCK)
approx_plan_kernel(const uint64_t* __restrict__ offs, uint64_t n_tasks, uint32_t strands, uint32_t chunk_len, uint64_t* __restrict__ cnt) {
    const uint64_t t = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (t < n_tasks) {
        const uint64_t read = strands == 2 ? t >> 1 : t;
        cnt[t] = apx_n_chunks((uint32_t)(offs[read + 1] - offs[read]), chunk_len);
    } else if (t == n_tasks) cnt[t] = 0;
}

// ck_off: the exclusive scan of the chunk counts, ckpt: ck_off[n_tasks] checkpoints (both nullptr where k = 0)
__global__ void __launch_bounds__(MS_BLOCK, APX_EXACT_MINW)
approx_exact_kernel(const moni_consts_t K, const moni_tables_t* __restrict__ T, const apx_args_t A, uint64_t n_tasks, const uint64_t* __restrict__ ck_off,
                    apx_ckpt_t* __restrict__ ckpt, unsigned long long* __restrict__ counters) {
    __shared__ lds_tables_t L;
    load_tables(L, T, K);
    const uint64_t t = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    loc_counts_t N; N.steps = N.rows = N.general = N.phi = 0;
    if (t < n_tasks) apx_exact(K, L, A, t, ckpt ? ckpt + ck_off[t] : nullptr, N);
    wave_add(N.steps, &counters[0]);
    wave_add(N.rows, &counters[1]);
    wave_add(N.general, &counters[3]);
}

// One lane per chunk of the batch, grid-stride (the grid is sized by an upper bound of the chunks and capped; the total is read from the scan).
__global__ void __launch_bounds__(MS_BLOCK, APX_MINW)
approx_tree_kernel(const moni_consts_t K, const moni_tables_t* __restrict__ T, const apx_args_t A, uint64_t n_tasks, const uint64_t* __restrict__ ck_off,
                   const apx_ckpt_t* __restrict__ ckpt, unsigned long long* __restrict__ counters) {
    __shared__ lds_tables_t L;
    __shared__ uint64_t stack[APX_STACK_LEVELS * APX_STACK_WORDS * MS_BLOCK];
    load_tables(L, T, K);
    const uint64_t total = ck_off[n_tasks];
    loc_counts_t N; N.steps = N.rows = N.general = N.phi = 0;
    unsigned long long rewalk = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x; g < total; g += (uint64_t)gridDim.x * MS_BLOCK) {
        const uint64_t t = apx_task_of(ck_off, n_tasks, g);
        const uint64_t o = ck_off[t];
        apx_piece(K, L, A, t, g - o, ckpt + o, stack + threadIdx.x, MS_BLOCK, N, rewalk);
    }
    wave_add(N.steps - rewalk, &counters[0]);
    wave_add(N.rows, &counters[1]);
    wave_add(N.general, &counters[3]);
}

// After the tree: n_kept = min(taken, max_hits), and the counts for the scan of the kept hits (thread n_tasks closes it)
__global__ void __launch_bounds__(MS_BLOCK)
approx_finish_kernel(uint64_t n_tasks, uint32_t max_hits, moni_approx_res_t* __restrict__ res, uint64_t* __restrict__ cnt) {
    const uint64_t t = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (t < n_tasks) {
        const uint32_t k = res[t].n_kept < max_hits ? res[t].n_kept : max_hits;
        res[t].n_kept = k;
        cnt[t] = k;
    } else if (t == n_tasks) cnt[t] = 0;
}

// One lane per slot of the region: slot j < n_kept of task t goes to hit_off[t] + j of the compact list; occ_cnt gets its n_occ for the scan
// (the lane of slot 0 closes it at hit_off[n_tasks]).
__global__ void __launch_bounds__(MS_BLOCK)
approx_gather_kernel(uint64_t n_tasks, uint32_t max_hits, moni_approx_res_t* __restrict__ res, const uint64_t* __restrict__ hit_off, uint32_t keep_toe,
                     const moni_approx_hit_t* __restrict__ slots, moni_approx_hit_t* __restrict__ hits, uint64_t* __restrict__ occ_cnt) {
    const uint64_t g = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (g == 0) occ_cnt[hit_off[n_tasks]] = 0;
    if (g >= n_tasks * max_hits) return;
    const uint64_t t = g / max_hits;
    const uint32_t j = (uint32_t)(g - t * max_hits);
    const uint64_t o = hit_off[t];
    if (j == 0) res[t].hit_off = o;
    if (j >= res[t].n_kept) return;
    moni_approx_hit_t H = slots[g];
    if (!keep_toe) H.occ_off = 0;                              // no walk will replace the toehold by the offset
    hits[o + j] = H;
    occ_cnt[o + j] = H.n_occ;
}

// off: the exclusive scan of the hits' n_occ (n_hits + 1 entries); pos / seq / seq_off hold off[n_hits] entries.  The toehold comes out of occ_off.
__global__ void __launch_bounds__(MS_BLOCK)
approx_walk_kernel(const moni_consts_t K, const phi_tab_t P, const uint64_t* __restrict__ seq_starts, uint64_t n_hits, moni_approx_hit_t* __restrict__ hits,
                   const uint64_t* __restrict__ off, uint64_t* __restrict__ pos, uint32_t* __restrict__ seq, uint64_t* __restrict__ seq_off,
                   unsigned long long* __restrict__ counters) {
    const uint64_t g = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    loc_counts_t N; N.steps = N.rows = N.general = N.phi = 0;
    if (g < n_hits) {
        const uint64_t toe = hits[g].occ_off, o = off[g];
        const uint32_t n_occ = hits[g].n_occ;
        hits[g].occ_off = o;
        if (n_occ) loc_walk(K, P, seq_starts, toe, n_occ, pos + o, seq + o, seq_off + o, N);
    }
    wave_add(N.phi, &counters[2]);
}
