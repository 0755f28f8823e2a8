// Per-lane logic of the loci query (per pattern and strand: the distinct reference positions its occurrences lift to, each with the number of
// occurrences that land there), host-compilable like seqcount_core.h (the kernels are in loci_kernels.hip, the host replay in
// tests/host_sim/loci_sim.cpp).
//
//   loci_key       one text position: liftidx::lift of it (the value ac_lift of align_core.h computes), or the position itself
//   loci_seg_hi    the upper rank of a segment of sc_segment: with it every position a segment walk yields knows its rank, and so its slot
//   loci_seg_keys  one segment: (task << 40) | key of every position, each at the slot of its rank
//   loci_is_head   one sorted key: the first of its locus
//
// The segments are seqcount's (sc_plan / sc_segment / sc_seg_walk).  A histogram by sequence can add atomically into a row; a list of loci cannot, but
// a segment knows the suffix-array ranks it covers: the occurrence of rank q of task t goes to slot occ_off[t] + (q - sa_lo), so the key buffer is
// complete and the same whatever order the lanes finish in.  The task in the high bits makes one sort of the whole buffer a sort per task, and the
// fold (heads, their scan, the differences of consecutive head indices) never looks at a segment boundary.
#pragma once
#include "lift_core.h"
#include "seqcount_core.h"

#define LOCI_POS_BITS 40u                                  // a key is a position in the concatenation: below 2^39 by the limits of the index image
#define LOCI_POS_MASK ((1ull << LOCI_POS_BITS) - 1)
#define LOCI_MAX_TASKS (1ull << (64 - LOCI_POS_BITS))      // the task index lies beside the position in a 64-bit sort key

// the lift tables of the index (lift_build.hpp): the directory is always there
struct loci_lift_t { const uint64_t* pdir; const moni_lift_seq_t* seqs; const moni_lift_run_t* runs; uint64_t n_text; uint32_t n_seq; };

// bits of the sort key that can differ: the position's, and as many as the largest task index has
MONI_HD uint32_t loci_key_bits(uint64_t n_tasks) {
    uint32_t b = 0;
    while (b < 64 - LOCI_POS_BITS && (1ull << b) < n_tasks) ++b;
    return LOCI_POS_BITS + b;
}

// liftidx::lift (liftidx.hpp:89-95) as ac_lift takes it: the directory entry of the position's block gives a sequence at or before the position's
// and a lift run at or before its haplotype offset; both are walked forward.  Where the sequence moved, the hint run is another sequence's and the
// run is searched (lift_pos).
MONI_HD uint64_t loci_key(const loci_lift_t& T, uint64_t pos, uint32_t lift) {
    if (!lift) return pos;
    uint64_t b = pos >> MONI_PDIR_SHIFT;
    const uint64_t nb = (T.n_text >> MONI_PDIR_SHIFT) + 1;
    if (b > nb) b = nb;
    const uint64_t e = T.pdir[b];
    uint32_t sid = (uint32_t)e;
    bool moved = false;
    while (sid + 1 < T.n_seq && pos >= T.seqs[sid + 1].start) { ++sid; moved = true; }
    const moni_lift_seq_t L = T.seqs[sid];
    const uint64_t start = pos - L.start;
    if (moved) return L.second + lift_pos(T.runs + L.run_off, L.n_runs, start);
    uint32_t k = (uint32_t)(e >> 32);
    const uint32_t last = L.run_off + L.n_runs;
    moni_lift_run_t R = T.runs[k];
    while (k + 1 < last) { const moni_lift_run_t N = T.runs[k + 1]; if ((uint64_t)N.hap > start) break; R = N; ++k; }
    return L.second + (uint64_t)R.ref + ((R.flags & MONI_LIFT_INS) ? 0ull : start - (uint64_t)R.hap);
}

// the highest rank of segment s of a task (sc_segment walks down from there): the interval's upper end for the last segment, else the last position of run k_lo + s
MONI_HD uint64_t loci_seg_hi(const moni_row_t* __restrict__ rows, uint64_t sa_lo, uint64_t count, uint32_t k_lo, uint32_t n_segs, uint32_t s) {
    return s + 1 == n_segs ? sa_lo + count - 1 : ld_start(rows, k_lo + s + 1) - 1;
}

// keys: the task's slots (keys[q - sa_lo] for rank q); hi_rel = the segment's upper rank - sa_lo
MONI_HD void loci_seg_keys(const moni_consts_t& K, const phi_tab_t P, const loci_lift_t& T, sc_seg_t G, uint64_t task, uint64_t hi_rel, uint32_t lift,
                           uint64_t* __restrict__ keys, unsigned long long& phi_steps) {
    uint64_t slot = hi_rel;
    sc_seg_walk(K, P, G, phi_steps, [&](uint64_t p) { keys[slot] = (task << LOCI_POS_BITS) | loci_key(T, p, lift); --slot; });
}

MONI_HD bool loci_is_head(const uint64_t* __restrict__ sorted, uint64_t i) { return i == 0 || sorted[i] != sorted[i - 1]; }
