// Per-lane logic of the sequence-count query (per pattern and strand: how many occurrences start in each sequence of the index), host-compilable
// like locate_core.h (the kernels are in seqcount_kernels.hip, the host replay in tests/host_sim/seqcount_sim.cpp).
//
//   sc_plan      one task: the BWT runs its interval [sa_lo, sa_lo + count - 1] touches; one segment per run
//   sc_segment   one segment: its ranks and the suffix-array value at its upper rank (the toehold)
//   sc_seg_walk  the positions of a segment, by phi from its toehold downwards, handed to a callback
//   sc_seg_count ... binned by sequence into the task's row of the table
//
// An occurrence list needs phi from one toehold, rank by rank: one lane per task.  A histogram does not care in which order the occurrences come, and
// the r-index samples the suffix array at the last position of every run: an interval that spans m runs has m toeholds, the task's own SA[hi] for the
// run of hi and samples_last of run k for every run k in front of it.  The image holds samples_last(k) - 1 as the esa field (w2) of
// recs[rec_base[head_k] + j + 1], j the number of head_k-runs in front of run k (the record of the NEXT head_k-run carries the sample of this one).
#pragma once
#include "locate_core.h"

// the per-code constants a segment needs, where a divergent index costs an LDS read (kernels) or nothing (host)
struct sc_tabs_t { uint32_t rec_base[MONI_MAX_SIGMA]; uint32_t hot_slot[MONI_MAX_SIGMA]; };

struct sc_seg_t { uint64_t toe; uint64_t len; };

// the run k < r with start[k] <= pos < start[k + 1], pos < n: a binary search over rows[].start
MONI_HD uint32_t sc_run_of(const moni_row_t* __restrict__ rows, uint64_t r, uint64_t pos) {
    uint32_t lo = 0, hi = (uint32_t)r;                       // start[lo] <= pos < start[hi]  (start[r] = n)
    while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (ld_start(rows, mid) <= pos) lo = mid; else hi = mid; }
    return lo;
}

// walked: the task is enumerated (max_walk == 0: no limit); n_segs = 0 where it is not, or has no occurrence
MONI_HD void sc_plan(const moni_consts_t& K, const moni_row_t* __restrict__ rows, uint64_t count, uint64_t sa_lo, uint64_t max_walk, uint32_t& k_lo,
                     uint32_t& n_segs, uint32_t& walked) {
    walked = (max_walk == 0 || count <= max_walk) ? 1u : 0u;
    k_lo = 0; n_segs = 0;
    if (!walked || !count) return;
    k_lo = sc_run_of(rows, K.r, sa_lo);
    const uint64_t hi = sa_lo + count - 1;
    const uint32_t k_hi = hi < ld_start(rows, k_lo + 1) ? k_lo : sc_run_of(rows, K.r, hi);
    n_segs = k_hi - k_lo + 1;
}

// segment s (0 .. n_segs - 1) of a task: the part of [sa_lo, hi] inside run k_lo + s
MONI_HD sc_seg_t sc_segment(const moni_consts_t& K, const sc_tabs_t& T, const moni_row_t* __restrict__ rows, const uint32_t* __restrict__ cr,
                            const moni_rec_t* __restrict__ recs, uint64_t sa_lo, uint64_t count, uint64_t task_toe, uint32_t k_lo, uint32_t n_segs, uint32_t s) {
    const uint32_t k = k_lo + s;
    const uint64_t hi = sa_lo + count - 1;
    const moni_row_t A = ld_row(rows, k);
    const uint64_t a = s == 0 ? sa_lo : row_start(A);
    sc_seg_t G;
    if (s + 1 == n_segs) { G.toe = task_toe; G.len = hi - a + 1; return G; }
    const uint64_t next = ld_start(rows, k + 1);
    G.len = next - a;
    const uint32_t h = row_head(A), hs = T.hot_slot[h];
    const uint32_t j = hs < 4 ? row_hot(A, hs) : cr[(uint64_t)k * K.sigma + h];
    const uint64_t e = recs[(uint64_t)T.rec_base[h] + j + 1].w2;          // SA[last position of run k] - 1 (mod n)
    G.toe = e + 1 == K.n ? 0 : e + 1;
    return G;
}

// len positions from the toehold downwards: emit(p) for each; phi is asked len - 1 times and never for a rank below the segment
template <class Emit>
MONI_HD void sc_seg_walk(const moni_consts_t& K, const phi_tab_t P, sc_seg_t G, unsigned long long& phi_steps, Emit emit) {
    uint64_t p = G.toe;
    for (uint64_t i = 0; i < G.len; ++i) {
        if (i) { uint64_t nxt, lcp; phi_step(P, K, p, nxt, lcp); p = nxt; ++phi_steps; }
        emit(p);
    }
}

// Add: row[seq] += v, atomically on the device.  A lane keeps the running (sequence, count) pair: neighbours in the suffix array are copies of one
// another in different sequences as often as not, but a flush per change is never more than one add per occurrence.
template <class Add>
MONI_HD void sc_seg_count(const moni_consts_t& K, const phi_tab_t P, const uint64_t* __restrict__ seq_starts, sc_seg_t G, unsigned long long& phi_steps, Add add) {
    uint32_t cur = 0xFFFFFFFFu;
    uint64_t run = 0;
    sc_seg_walk(K, P, G, phi_steps, [&](uint64_t p) {
        const uint32_t sid = seq_of(seq_starts, K.n_seq, p);
        if (sid != cur) { if (run) add(cur, run); cur = sid; run = 0; }
        ++run;
    });
    if (run) add(cur, run);
}

// the task of global segment g: the last t with off[t] <= g (off: exclusive scan of n_segs, n_tasks + 1 entries, g < off[n_tasks])
MONI_HD uint64_t sc_task_of(const uint64_t* __restrict__ off, uint64_t n_tasks, uint64_t g) {
    uint64_t lo = 0, hi = n_tasks;                            // off[lo] <= g < off[hi]
    while (hi - lo > 1) { const uint64_t mid = lo + ((hi - lo) >> 1); if (off[mid] <= g) lo = mid; else hi = mid; }
    return lo;
}
