// HIP kernels (gfx950) of matching statistics of long patterns (moni_ms_long_batch); the per-lane logic and the method are in mslong_core.h.
// Included from moni_hip.hip after seed_kernels.hip (MS_BLOCK, load_tables, wave_add).
//
// Mapping: one LANE per segment for the speculative walk and the first length pass - a 60 Mbase pattern cut every 4096 bases gives 15 000 walks
// that are independent, where ms_lf_kernel has one - and one lane per run of flagged segments for the chain re-walk and its length pass.  The
// segment table and the list of runs are made on the device (a count per pattern, an exclusive scan, one lane per segment); the host reads back
// two counts to size the launches.  Pointers and lengths go to plain arrays in pattern order (8 + 4 bytes per base): 8 pointers as one aligned
// 64-byte group, 4 lengths as one 16-byte store, value by value at a segment's edges.
#include "mslong_core.h"

#define MSLONG_MINW 8       // waves per SIMD the register allocator must leave room for, as pml_kernel

// cnt[i] = segments of pattern i; cnt[n_pat] = 0 (the exclusive scan's total lands there)
extern "C" __global__ void __launch_bounds__(256) mslong_count_kernel(const uint64_t* __restrict__ offs, uint64_t n_pat, uint32_t seg_len, uint64_t* __restrict__ cnt) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_pat) cnt[i] = mslong_n_segs(offs[i] - offs[0], offs[i + 1] - offs[i], seg_len);
    if (i == n_pat) cnt[i] = 0;
}

// one lane per segment: its pattern by binary search over the scanned counts (seg_off[i] = first segment of pattern i; n_pat + 1 entries)
extern "C" __global__ void __launch_bounds__(256) mslong_table_kernel(const uint64_t* __restrict__ offs, const uint64_t* __restrict__ seg_off, uint64_t n_pat, uint64_t n_segs,
                                                                      uint32_t seg_len, uint32_t overlap, mslong_seg_t* __restrict__ segs, uint32_t* __restrict__ flags) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_segs) return;
    uint64_t lo = 0, hi = n_pat;                            // the last i with seg_off[i] <= s (patterns without segments share their successor's offset)
    while (hi - lo > 1) { const uint64_t mid = lo + ((hi - lo) >> 1); if (seg_off[mid] <= s) lo = mid; else hi = mid; }
    segs[s] = mslong_seg((uint32_t)lo, offs[lo] - offs[0], offs[lo + 1] - offs[lo], seg_len, overlap, s - seg_off[lo]);
    flags[s] = 0;
}

// counters: [0] steps of the speculative walk, [1] threshold jumps (both rounds), [2] steps of the chain re-walk, [3] flagged segments, [4] their bases
__global__ void __launch_bounds__(MS_BLOCK, MSLONG_MINW)
mslong_walk_kernel(const moni_consts_t K, const moni_tables_t* __restrict__ T, const moni_row_t* __restrict__ rows, const moni_frow_t* __restrict__ frows,
                   const uint32_t* __restrict__ cr, const moni_rec_t* __restrict__ recs, const uint8_t* __restrict__ seq, const uint64_t* __restrict__ offs,
                   const mslong_seg_t* __restrict__ segs, uint64_t n_segs, uint64_t* __restrict__ ptr, mslong_state_t* __restrict__ states,
                   unsigned long long* __restrict__ counters) {
    __shared__ lds_tables_t L;
    __shared__ uint32_t GLO[8][MS_BLOCK];
    __shared__ uint8_t GHI[8][MS_BLOCK];
    load_tables(L, T, K);
    mslong_grp_t G; G.lo = &GLO[0][threadIdx.x]; G.hi = &GHI[0][threadIdx.x]; G.stride = MS_BLOCK;
    const uint64_t s = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    unsigned long long n_steps = 0, n_jumps = 0;
    if (s < n_segs) {
        const mslong_seg_t g = segs[s];
        const uint64_t off = offs[g.pat];
        mslong_walk(K, L, rows, frows, cr, recs, seq, off, off - offs[0], g.a, g.b, g.e, nullptr, ptr, states + s, G, n_steps, n_jumps);
    }
    wave_add(n_steps, &counters[0]);
    wave_add(n_jumps, &counters[1]);
}

// round 1: one lane per segment; flags[s] = 1 where the comparison reached the walk's first position
__global__ void __launch_bounds__(MS_BLOCK)
mslong_len_kernel(const moni_consts_t K, const uint8_t* __restrict__ text, const uint8_t* __restrict__ seq, const uint64_t* __restrict__ offs,
                  const mslong_seg_t* __restrict__ segs, uint64_t n_segs, const uint64_t* __restrict__ ptr, uint32_t* __restrict__ lens, uint32_t* __restrict__ flags,
                  unsigned long long* __restrict__ counters) {
    const uint64_t s = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    unsigned long long n_flag = 0, n_bases = 0;
    if (s < n_segs) {
        const mslong_seg_t g = segs[s];
        const uint64_t off = offs[g.pat];
        const uint32_t m = (uint32_t)(offs[g.pat + 1] - off);
        const uint64_t reach = mslong_len(K, text, seq, off, off - offs[0], g.a, g.b, g.e, m, ptr, lens);
        if (g.e < m && reach >= g.e) { flags[s] = 1; n_flag = 1; n_bases = g.b - g.a; }
    }
    wave_add(n_flag, &counters[3]);
    wave_add(n_bases, &counters[4]);
}

// head[s] = 1 where a run of flagged segments begins (the last segment of a pattern is never flagged, so a run never crosses into the next pattern)
extern "C" __global__ void __launch_bounds__(256) mslong_head_kernel(const uint32_t* __restrict__ flags, uint64_t n_segs, uint64_t* __restrict__ head) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s < n_segs) head[s] = (flags[s] && (s == 0 || !flags[s - 1])) ? 1 : 0;
    if (s == n_segs) head[s] = 0;
}
// run_idx: the exclusive scan of head; the lane of a run's first segment looks for its last one
extern "C" __global__ void __launch_bounds__(256) mslong_runs_kernel(const uint32_t* __restrict__ flags, uint64_t n_segs, const uint64_t* __restrict__ run_idx,
                                                                     mslong_run_t* __restrict__ runs) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_segs || !flags[s] || (s > 0 && flags[s - 1])) return;
    uint64_t t = s;
    while (t + 1 < n_segs && flags[t + 1]) ++t;
    mslong_run_t r; r.s0 = (uint32_t)s; r.s1 = (uint32_t)t;
    runs[run_idx[s]] = r;
}

// round 2: one lane per run, from the state the segment behind the run saved at its first base down to the run's first base
__global__ void __launch_bounds__(MS_BLOCK, MSLONG_MINW)
mslong_chain_kernel(const moni_consts_t K, const moni_tables_t* __restrict__ T, const moni_row_t* __restrict__ rows, const moni_frow_t* __restrict__ frows,
                    const uint32_t* __restrict__ cr, const moni_rec_t* __restrict__ recs, const uint8_t* __restrict__ seq, const uint64_t* __restrict__ offs,
                    const mslong_seg_t* __restrict__ segs, uint64_t n_segs, const mslong_run_t* __restrict__ runs, uint64_t n_runs, uint64_t* __restrict__ ptr,
                    const mslong_state_t* __restrict__ states, unsigned long long* __restrict__ counters) {
    __shared__ lds_tables_t L;
    __shared__ uint32_t GLO[8][MS_BLOCK];
    __shared__ uint8_t GHI[8][MS_BLOCK];
    load_tables(L, T, K);
    mslong_grp_t G; G.lo = &GLO[0][threadIdx.x]; G.hi = &GHI[0][threadIdx.x]; G.stride = MS_BLOCK;
    const uint64_t t = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    unsigned long long n_steps = 0, n_jumps = 0;
    if (t < n_runs) {
        const mslong_run_t r = runs[t];
        if ((uint64_t)r.s1 + 1 < n_segs) {                  // (always: a flagged segment has e < m, so its pattern has a segment behind it)
            const mslong_seg_t g0 = segs[r.s0], g1 = segs[r.s1];
            const uint64_t off = offs[g0.pat];
            mslong_walk(K, L, rows, frows, cr, recs, seq, off, off - offs[0], g0.a, g1.b, g1.b, states + r.s1 + 1, ptr, nullptr, G, n_steps, n_jumps);
        }
    }
    wave_add(n_steps, &counters[2]);
    wave_add(n_jumps, &counters[1]);
}

__global__ void __launch_bounds__(MS_BLOCK)
mslong_relen_kernel(const moni_consts_t K, const uint8_t* __restrict__ text, const uint8_t* __restrict__ seq, const uint64_t* __restrict__ offs,
                    const mslong_seg_t* __restrict__ segs, const mslong_run_t* __restrict__ runs, uint64_t n_runs, const uint64_t* __restrict__ ptr,
                    uint32_t* __restrict__ lens) {
    const uint64_t t = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (t >= n_runs) return;
    const mslong_run_t r = runs[t];
    const mslong_seg_t g0 = segs[r.s0], g1 = segs[r.s1];
    const uint64_t off = offs[g0.pat];
    const uint32_t m = (uint32_t)(offs[g0.pat + 1] - off);
    (void)mslong_len(K, text, seq, off, off - offs[0], g0.a, g1.b, m, m, ptr, lens);
}
