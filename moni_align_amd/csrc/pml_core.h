// Per-lane logic of pseudo-matching lengths (PML), the legacy `moni pseudo-ms` of SPUMONI: host-compilable like seed_core.h (the kernel is in
// pml_kernels.hip, the host replay in tests/host_sim/pml_sim.cpp).
//
//   pml_task   ms_pointers<sparse_sd_vector, ms_rle_string_sd, thr_bv<>>::_query   include/ms/spumoni.hpp:356-410
//              (called per read by src/spumoni/run_spumoni.cpp:186-193)
//
// The walk over BWT positions is the one of ms_task (include/ms/moni.hpp:568-624) step for step: same start, same match test, same threshold
// jumps.  What differs: no suffix-array sample is carried (a jump reads the slot word only, not the sample words of the fast row), the value
// per step is one counter - length + 1 on a match, 0 on a jump or on a byte whose letter the BWT does not hold - and only the forward strand
// is walked.  Row fields are decoded with the accessors of seed_core.h / layout.h.
#pragma once
#include "seed_core.h"

// The general path of one step: absolute position, rows / cr / recs (spumoni.hpp:378-404).  Returns bwt[pos] == c.
MONI_HD bool pml_step_general(const moni_consts_t& K, const lds_tables_t& L, const moni_row_t* __restrict__ rows, const uint32_t* __restrict__ cr,
                              const moni_rec_t* __restrict__ recs, uint32_t c, ms_state_t& S, unsigned long long& n_jumps) {
    moni_row_t A;
    settle_run(rows, K.r, S.pos, S.run, A);
    S.abs = true;
    if (row_head(A) == c) {                                  // bwt[pos] == c  (spumoni.hpp:378-383); the sentinel head never matches
        S.pos = row_lfbase(A) + (S.pos - row_start(A));
        S.run = row_dest(A);
        return true;
    }
    ++n_jumps;                                               // threshold jump (spumoni.hpp:384-404)
    const uint32_t hs = L.hot_slot[c];
    const uint32_t j = hs < 4 ? row_hot(A, hs) : cr[(uint64_t)S.run * K.sigma + c];
    const moni_u64x4 rv = *reinterpret_cast<const moni_u64x4*>(recs + L.rec_base[c] + j);
    const uint64_t thr = rv.x & MONI_POS_MASK;
    // rnk_c.first > thresholds.rank(pos+1, c)  <=>  j >= 1 and (no c-run below, or pos < thr_j)
    const bool up = j > 0 && (j == L.rec_cnt[c] || S.pos < thr);
    S.pos = up ? rv.w - 1 : rv.w;                            // F[c] + rnk_c.second (- 1)
    S.run = (uint32_t)((rv.x >> 40) << 24) | (uint32_t)(rv.y >> 40);
    return false;
}

// One backward step of one read for symbol code c; the state is ms_state_t's (run, off) or absolute position, its sample unused.
// Returns whether the step was a match (bwt[pos] == c).
MONI_HD bool pml_step(const moni_consts_t& K, const lds_tables_t& L, const moni_row_t* __restrict__ rows, const moni_frow_t* __restrict__ frows,
                      const uint32_t* __restrict__ cr, const moni_rec_t* __restrict__ recs, uint32_t c, ms_state_t& S, unsigned long long& n_jumps) {
    if (S.abs) {                                             // re-anchor an absolute position: (run, off)
        moni_row_t A;
        settle_run(rows, K.r, S.pos, S.run, A);
        S.off = (uint32_t)(S.pos - row_start(A));
        if (S.pos - row_start(A) >= MONI_ROW_LEN_SAT) return pml_step_general(K, L, rows, cr, recs, c, S, n_jumps);
        S.abs = false;
    }
    const uint32_t hc = L.hot_slot[c];
    while (true) {
        const moni_frow_t* __restrict__ fr = frows + S.run;
        const uint64_t w0 = fr->w[0];
        const uint32_t len = (uint32_t)w0 & 0xFFFu;
        if (!((w0 >> 58) & 1u) || hc >= 4) {                 // general path: absolute position from the 32-byte row
            if (S.off == MONI_OFF_END) S.pos = ld_start(rows, S.run + 1) - 1;
            else S.pos = ld_start(rows, S.run) + S.off;
            return pml_step_general(K, L, rows, cr, recs, c, S, n_jumps);
        }
        if (S.off == MONI_OFF_END) S.off = len - 1;
        if (S.off >= len) { S.off -= len; ++S.run; continue; }          // the LF image ran past the destination run: next run
        const uint32_t hh = (uint32_t)(w0 >> 56) & 3u;
        if (hc == hh) {                                      // bwt[pos] == c
            S.off += (uint32_t)(w0 >> 12) & 0xFFFu;
            S.run = (uint32_t)(w0 >> 24);
            return true;
        }
        ++n_jumps;
        const uint32_t sl = (hc - hh - 1u) & 3u;             // 0..2
        const uint64_t ws = fr->w[1 + sl];                   // the slot word alone: thr_off | sdoff | sdest (the samples in w4..w7 are not read)
        const uint32_t thr_off = (uint32_t)ws & 0xFFFu;
        const uint32_t sdoff = (uint32_t)(ws >> 12) & 0xFFFu;
        const uint32_t sdest = (uint32_t)(ws >> 24);
        if (S.off < thr_off) {                               // jump up: last position of the previous c-run
            if (sdoff == 0) { S.run = sdest - 1; S.off = MONI_OFF_END; }
            else { S.run = sdest; S.off = sdoff - 1; }
        } else {                                             // jump down: first position of the next c-run
            S.run = sdest; S.off = sdoff;
        }
        return false;
    }
}

// four lengths to p (on the device p is 16-byte aligned: one store)
MONI_HD void pml_store4(uint32_t* __restrict__ p, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
#if defined(__HIP_DEVICE_COMPILE__)
    moni_u64x2 v; v.x = (uint64_t)a | ((uint64_t)b << 32); v.y = (uint64_t)c | ((uint64_t)d << 32);
    *reinterpret_cast<moni_u64x2*>(p) = v;
#else
    p[0] = a; p[1] = b; p[2] = c; p[3] = d;
#endif
}

// One read, forward strand, bytes as they are: lens[offs[read] - offs[0] + k] = PML at read offset k; read_max[read] = the largest of them
// (0 for an empty read), read_hits[read] = the number of offsets with PML >= thr.  The pattern comes from pack_task's workspace (task 2 * read).
MONI_HD void pml_task(const moni_consts_t& K, const lds_tables_t& L, const moni_row_t* __restrict__ rows, const moni_frow_t* __restrict__ frows,
                      const uint32_t* __restrict__ cr, const moni_rec_t* __restrict__ recs, const uint64_t* __restrict__ pat,
                      const uint64_t* __restrict__ offs, const moni_u64x2* __restrict__ blk, uint64_t read, uint32_t thr, uint32_t* __restrict__ lens,
                      uint32_t* __restrict__ read_max, uint32_t* __restrict__ read_hits, unsigned long long& n_steps, unsigned long long& n_jumps) {
    const uint64_t off = offs[read];
    const uint32_t m = (uint32_t)(offs[read + 1] - off);
    const uint64_t pb = ws_pat_base(blk, 2 * read);
    uint32_t* __restrict__ out = lens + (off - offs[0]);
    ms_state_t S;
    S.run = (uint32_t)K.r - 1; S.pos = K.n - 1; S.abs = true; S.off = 0; S.m = m;     // start with the empty string
    S.sample = 0; S.word = 0;
    uint32_t length = 0, mx = 0, hits = 0;
    // The lengths of four neighbouring places of `lens` are collected in registers and stored together where the group lies inside the read
    // (16 bytes, aligned: a quarter of the store requests); the groups a read shares with its neighbours are stored value by value.
    const uint64_t g0 = off - offs[0];
    uint32_t q0 = 0, q1 = 0, q2 = 0, q3 = 0;
    for (uint32_t s = 0; s < m; ++s) {
        if ((s & 7u) == 0) S.word = pat[pb + (uint64_t)(s >> 3) * 64u];               // pattern[m-1-s]
        const uint32_t raw = (uint32_t)S.word & 0xFFu;
        S.word >>= 8;
        const uint32_t c = L.code[raw];
        if (c == MONI_CODE_ABSENT) {                          // n_c == 0   (spumoni.hpp:372-377)
            length = 0;
            S.pos = L.abs_pos[raw];
            S.run = L.abs_run[raw];
            S.abs = true;
        } else {
            length = pml_step(K, L, rows, frows, cr, recs, c, S, n_jumps) ? length + 1 : 0;
        }
        {
            const uint32_t k = m - 1 - s;
            const uint32_t ln4 = (uint32_t)(g0 + k) & 3u;
            if (ln4 == 0) q0 = length; else if (ln4 == 1) q1 = length; else if (ln4 == 2) q2 = length; else q3 = length;
            if (ln4 == 0) {
                if (k + 3 < m) pml_store4(out + k, q0, q1, q2, q3);
                else { out[k] = q0; if (k + 1 < m) out[k + 1] = q1; if (k + 2 < m) out[k + 2] = q2; }
            }
        }
        mx = length > mx ? length : mx;
        hits += length >= thr ? 1u : 0u;
    }
    {   // the group that holds read offset 0 begins in front of the read: its values were not stored above
        const uint32_t r = (uint32_t)g0 & 3u;
        if (r == 1) { if (m > 0) out[0] = q1; if (m > 1) out[1] = q2; if (m > 2) out[2] = q3; }
        else if (r == 2) { if (m > 0) out[0] = q2; if (m > 1) out[1] = q3; }
        else if (r == 3) { if (m > 0) out[0] = q3; }
    }
    read_max[read] = mx;
    read_hits[read] = hits;
    n_steps += m;
}
