// Per-lane logic of the exact-match queries (count and locate: what ri::r_index::count / locate_all give the reference's C++ users through
// ms_pointers), host-compilable like seed_core.h and pml_core.h (the kernels are in locate_kernels.hip, the host replay in
// tests/host_sim/locate_sim.cpp).
//
//   loc_step   one backward-search step of the interval [lo, hi] with the toehold SA[hi]
//   loc_task   the search of one (pattern, strand): count, first BWT position, bytes matched, toehold
//   loc_walk   the positions of the n_occ highest ranks of the interval, by phi from the toehold, with sequence index and offset
//
// The index image holds the LF images a backward search needs.  For a position of a run whose head is not c, the fast row's slot of c stores
// (sdest, sdoff) = F[c] + rank_c(position): the LF image of the first position of the next c-run - the new lower end - and one before it is the image of
// the last c above - the new upper end, whose suffix-array value is the slot's esa.  The general path has the same values as lfpos / esa in recs.
// Nothing of the interval is ever an absolute position on the fast path: both ends are (run, offset), the interval is empty exactly when neither
// end's head is c and both ends see the same next c-run, and rows[].start is read once, at the end, for the count.
#pragma once
#include "seed_core.h"

struct loc_end_t { uint64_t pos; uint32_t run, off; };       // (run, off) - off may be MONI_OFF_END or lie past the run - or, loc_state_t::abs, the absolute position pos (run: a guess)
struct loc_state_t {
    loc_end_t lo, hi;                // the interval, hi inclusive
    uint64_t toe;                    // SA[hi]
    bool abs;
};
// what a walk adds to the context's counters
struct loc_counts_t { unsigned long long steps, rows, general, phi; };

MONI_HD uint64_t loc_abs(const moni_row_t* __restrict__ rows, const loc_end_t& E) {
    return E.off == MONI_OFF_END ? ld_start(rows, E.run + 1) - 1 : ld_start(rows, E.run) + E.off;
}

// The general path of one step: absolute positions, rows / cr / recs.  Returns whether the new interval holds a position.
MONI_HD bool loc_step_general(const moni_consts_t& K, const lds_tables_t& L, const moni_row_t* __restrict__ rows, const uint32_t* __restrict__ cr,
                              const moni_rec_t* __restrict__ recs, uint32_t c, loc_state_t& S, loc_counts_t& N) {
    ++N.general;
    S.abs = true;
    const uint32_t hs = L.hot_slot[c];
    moni_row_t A;
    uint64_t nlo, nhi, ntoe;
    uint32_t rlo, rhi;
    settle_run(rows, K.r, S.lo.pos, S.lo.run, A);
    if (row_head(A) == c) {                                  // LF of the position
        nlo = row_lfbase(A) + (S.lo.pos - row_start(A));
        rlo = row_dest(A);
    } else {                                                 // the image of the next c-run's first position
        const uint32_t j = hs < 4 ? row_hot(A, hs) : cr[(uint64_t)S.lo.run * K.sigma + c];
        const moni_u64x4 rv = *reinterpret_cast<const moni_u64x4*>(recs + L.rec_base[c] + j);
        nlo = rv.w;
        rlo = (uint32_t)((rv.x >> 40) << 24) | (uint32_t)(rv.y >> 40);
    }
    settle_run(rows, K.r, S.hi.pos, S.hi.run, A);
    if (row_head(A) == c) {
        nhi = row_lfbase(A) + (S.hi.pos - row_start(A));
        rhi = row_dest(A);
        ntoe = S.toe - 1;
    } else {                                                 // one before that image: the last c above, whose sample is the esa of the c-run in front
        const uint32_t j = hs < 4 ? row_hot(A, hs) : cr[(uint64_t)S.hi.run * K.sigma + c];
        const moni_u64x4 rv = *reinterpret_cast<const moni_u64x4*>(recs + L.rec_base[c] + j);
        nhi = rv.w - 1;                                      // F[c] >= 1: position 0 holds the terminator's suffix
        rhi = (uint32_t)((rv.x >> 40) << 24) | (uint32_t)(rv.y >> 40);
        ntoe = rv.z;
    }
    if (nlo > nhi) return false;
    S.lo.pos = nlo; S.lo.run = rlo; S.hi.pos = nhi; S.hi.run = rhi; S.toe = ntoe;
    return true;
}

// Brings (run, off) to an offset inside its run and reads the run's w0; the row of run `have` is already in have_w0 (0xFFFFFFFF: none).
// false: the row is not "ok" (the step takes the general path).
MONI_HD bool loc_anchor(const moni_frow_t* __restrict__ frows, loc_end_t& E, uint64_t& w0, uint32_t have, uint64_t have_w0, loc_counts_t& N) {
    while (true) {
        if (E.run == have) w0 = have_w0;
        else { w0 = frows[E.run].w[0]; ++N.rows; }
        if (!((w0 >> 58) & 1u)) return false;                // (the sentinel rows are not ok: the walk over runs ends there at the latest)
        const uint32_t len = (uint32_t)w0 & 0xFFFu;
        if (E.off == MONI_OFF_END) E.off = len - 1;
        if (E.off < len) return true;
        E.off -= len; ++E.run;                               // the LF image ran past the destination run: next run
    }
}

// One backward-search step for symbol code c.  Returns whether the new interval holds a position; if not, S is not to be used again.
MONI_HD bool loc_step(const moni_consts_t& K, const lds_tables_t& L, const moni_row_t* __restrict__ rows, const moni_frow_t* __restrict__ frows,
                      const uint32_t* __restrict__ cr, const moni_rec_t* __restrict__ recs, uint32_t c, loc_state_t& S, loc_counts_t& N) {
    ++N.steps;
    if (S.abs) {                                             // re-anchor absolute positions: (run, off)
        moni_row_t A;
        settle_run(rows, K.r, S.lo.pos, S.lo.run, A);
        const uint64_t ol = S.lo.pos - row_start(A);
        settle_run(rows, K.r, S.hi.pos, S.hi.run, A);
        const uint64_t oh = S.hi.pos - row_start(A);
        if (ol >= MONI_ROW_LEN_SAT || oh >= MONI_ROW_LEN_SAT) return loc_step_general(K, L, rows, cr, recs, c, S, N);
        S.lo.off = (uint32_t)ol; S.hi.off = (uint32_t)oh;
        S.abs = false;
    }
    const uint32_t hc = L.hot_slot[c];
    uint64_t wl = 0, wh = 0;
    const bool ok = hc < 4 && loc_anchor(frows, S.lo, wl, 0xFFFFFFFFu, 0, N) && loc_anchor(frows, S.hi, wh, S.lo.run, wl, N);
    if (!ok) {                                               // general path: absolute positions from the 32-byte rows
        S.lo.pos = loc_abs(rows, S.lo);
        S.hi.pos = loc_abs(rows, S.hi);
        return loc_step_general(K, L, rows, cr, recs, c, S, N);
    }
    const uint32_t hl = (uint32_t)(wl >> 56) & 3u, hh = (uint32_t)(wh >> 56) & 3u;
    if (S.lo.run == S.hi.run) {                              // both ends in one run: every position holds c, or none does
        if (hl != hc) return false;
        const uint32_t doff = (uint32_t)(wl >> 12) & 0xFFFu;
        S.lo.off += doff; S.hi.off += doff;
        S.lo.run = S.hi.run = (uint32_t)(wl >> 24);
        S.toe--;
        return true;
    }
    const uint32_t sll = (hc - hl - 1u) & 3u, slh = (hc - hh - 1u) & 3u;          // 0..2 where the head is not c
    uint64_t sl_lo = 0, sl_hi = 0;                           // the slot words: thr_off | sdoff | sdest | ssa_hi
    if (hl != hc) sl_lo = frows[S.lo.run].w[1 + sll];
    if (hh != hc) sl_hi = frows[S.hi.run].w[1 + slh];
    // neither end holds c and both see the same next c-run: no c in between
    if (hl != hc && hh != hc && ((sl_lo ^ sl_hi) & 0x00FFFFFFFFFFF000ull) == 0) return false;
    if (hl == hc) {
        S.lo.off += (uint32_t)(wl >> 12) & 0xFFFu;
        S.lo.run = (uint32_t)(wl >> 24);
    } else {
        S.lo.off = (uint32_t)(sl_lo >> 12) & 0xFFFu;
        S.lo.run = (uint32_t)(sl_lo >> 24);
    }
    if (hh == hc) {
        S.hi.off += (uint32_t)(wh >> 12) & 0xFFFu;
        S.hi.run = (uint32_t)(wh >> 24);
        S.toe--;
    } else {                                                 // the last position of the c-run above: one before (sdest, sdoff), sample esa
        const moni_frow_t* __restrict__ fr = frows + S.hi.run;
        const uint64_t e = slh == 0 ? (fr->w[5] >> 32) : slh == 1 ? (fr->w[6] & 0xFFFFFFFFull) : (fr->w[6] >> 32);
        S.toe = e | (((fr->w[7] >> (8 * slh)) & 0xFFull) << 32);
        const uint32_t sdoff = (uint32_t)(sl_hi >> 12) & 0xFFFu, sdest = (uint32_t)(sl_hi >> 24);
        if (sdoff == 0) { S.hi.run = sdest - 1; S.hi.off = MONI_OFF_END; }
        else { S.hi.run = sdest; S.hi.off = sdoff - 1; }
    }
    return true;
}

// One (pattern, strand): the pattern comes from pack_task's workspace (task 2 * read + strand), its bytes as they are - a byte <= 1 (terminator,
// separator) or one the BWT does not hold ends the search.  R.occ_off is left to the scan; *toe = SA[upper end] where R.count > 0.
MONI_HD void loc_task(const moni_consts_t& K, const lds_tables_t& L, const moni_row_t* __restrict__ rows, const moni_frow_t* __restrict__ frows,
                      const uint32_t* __restrict__ cr, const moni_rec_t* __restrict__ recs, const uint64_t* __restrict__ pat,
                      const uint64_t* __restrict__ offs, const moni_u64x2* __restrict__ blk, uint64_t read, uint32_t strand, uint32_t max_occ,
                      moni_locate_res_t& R, uint64_t& toe, loc_counts_t& N) {
    const uint32_t m = (uint32_t)(offs[read + 1] - offs[read]);
    const uint64_t pb = ws_pat_base(blk, 2 * read + strand);
    loc_state_t S;
    S.lo.pos = 0; S.lo.run = 0; S.lo.off = 0;                                    // [0, n): position 0 of run 0, the last position of run r - 1
    S.hi.pos = K.n - 1; S.hi.run = (uint32_t)K.r - 1; S.hi.off = MONI_OFF_END;
    S.toe = K.last_run_sample; S.abs = false;
    uint32_t matched = 0;
    uint64_t word = 0;
    bool alive = m > 0;
    for (uint32_t s = 0; s < m; ++s) {
        if ((s & 7u) == 0) word = pat[pb + (uint64_t)(s >> 3) * 64u];           // pattern[m-1-s], strand-resolved by pack_task
        const uint32_t raw = (uint32_t)word & 0xFFu;
        word >>= 8;
        const uint32_t c = L.code[raw];
        if (raw <= 1u || c == MONI_CODE_ABSENT || !loc_step(K, L, rows, frows, cr, recs, c, S, N)) { alive = false; break; }
        ++matched;
    }
    R.count = 0; R.sa_lo = 0; R.occ_off = 0; R.n_occ = 0; R.matched = matched;
    toe = 0;
    if (alive) {
        const uint64_t lo = S.abs ? S.lo.pos : loc_abs(rows, S.lo), hi = S.abs ? S.hi.pos : loc_abs(rows, S.hi);
        R.count = hi - lo + 1; R.sa_lo = lo;
        R.n_occ = R.count < max_occ ? (uint32_t)R.count : max_occ;
        toe = S.toe;
    }
}

// The n_occ highest ranks of an interval, in decreasing rank order: SA[hi] is the toehold, phi turns SA[i] into SA[i - 1].  The interval bounds the
// walk (n_occ <= count), so phi is never asked for the suffix of rank 0 and the LCP field of its records is not looked at.
MONI_HD void loc_walk(const moni_consts_t& K, const phi_tab_t P, const uint64_t* __restrict__ seq_starts, uint64_t toe, uint32_t n_occ,
                      uint64_t* __restrict__ pos, uint32_t* __restrict__ seq, uint64_t* __restrict__ seq_off, loc_counts_t& N) {
    uint64_t p = toe;
    for (uint32_t i = 0; i < n_occ; ++i) {
        if (i) { uint64_t nxt, lcp; phi_step(P, K, p, nxt, lcp); p = nxt; ++N.phi; }
        const uint32_t sid = seq_of(seq_starts, K.n_seq, p);          // seqidx::index (seqidx.hpp:149-154), no lift-over
        pos[i] = p; seq[i] = sid; seq_off[i] = p - seq_starts[sid];
    }
}
