// Per-lane logic of read screening: host-compilable like pml_core.h (the kernel is in screen_kernels.hip, the host replay in
// tests/host_sim/screen_sim.cpp).  The walk is pml_task's, step for step (pml_step / pml_step_general, the accessors of seed_core.h); what is
// new is what happens to the lengths: none is stored.
//
// One lane walks ONE of the four strings of a read; the lanes of a read are neighbours, role = lane & 3 (with one strand: lane & 1):
//   role 0  P0  the read's bytes as they are            role 1  N0 = reverse(P0)
//   role 2  P1  the reverse complement (pack_task's)    role 3  N1 = reverse(P1)
// A null lane needs no packing of its own: step s of N consumes N[m-1-s] = P[s], the byte P's lane consumes at step m-1-s - the same packed words
// read from the other end.  All lanes of a read take m steps and stand at offset m-1-s of their own string at step s, so a window closes for all
// of them in the same step.
//
// Each lane keeps the histogram of its current window in a column of its own: MONI_SCREEN_BINS 16-bit bins, two to a 32-bit word (a window has at
// most 65535 offsets: a bin cannot carry into its neighbour).  At a window's end the pattern lane takes the null lane's words through X.pair()
// and folds the two columns into D with a prefix loop over the bins; the pattern lane of strand 1 hands its three figures to the lane of strand 0
// through X.strand(), which writes the read's record - the only value that leaves the lane.
//   X.pair(w)    the value w of the lane with role ^ 1 (device: a cross-lane move; host replay: a log the null lane filled when it ran first)
//   X.strand(v)  the value v of the lane with role ^ 2
#pragma once
#include "pml_core.h"

#define SCREEN_WORDS (MONI_SCREEN_BINS / 2)

// window, min_win, ks_num / ks_den and strands inside their ranges, the reserved words zero
MONI_HD bool screen_params_ok(const moni_screen_params_t& p) {
    return p.window >= 8 && p.window <= 65535 && p.min_win >= 1 && p.min_win <= p.window && p.ks_num >= 1 && p.ks_num <= p.ks_den && p.ks_den <= 65535 &&
           (p.strands == 1 || p.strands == 2) && !p.reserved[0] && !p.reserved[1] && !p.reserved[2];
}

// scored windows of a read of m offsets: the full ones, and the last one where it holds at least min_win offsets
MONI_HD uint32_t screen_n_win(uint32_t m, const moni_screen_params_t& p) { return m / p.window + (m % p.window >= p.min_win ? 1u : 0u); }

// One more value of the two running sums: D = max(D, #{b <= v} - #{a <= v})
MONI_HD void screen_ks_bin(uint32_t a, uint32_t b, uint32_t& cum_a, uint32_t& cum_b, uint32_t& D) {
    cum_a += a; cum_b += b;
    const int32_t d = (int32_t)(cum_b - cum_a);
    D = d > (int32_t)D ? (uint32_t)d : D;
}

MONI_HD void screen_store(moni_screen_res_t* __restrict__ p, const moni_screen_res_t& r) {
#if defined(__HIP_DEVICE_COMPILE__)
    moni_u64x2 lo, hi;      // two 16-byte vector stores (the records are 32-byte aligned)
    lo.x = (uint64_t)r.n_win | ((uint64_t)r.n_pos[0] << 32); lo.y = (uint64_t)r.n_pos[1] | ((uint64_t)r.d_max[0] << 32);
    hi.x = (uint64_t)r.d_max[1] | ((uint64_t)r.max_pml[0] << 32); hi.y = (uint64_t)r.max_pml[1] | ((uint64_t)r.flags << 32);
    reinterpret_cast<moni_u64x2*>(p)[0] = lo;
    reinterpret_cast<moni_u64x2*>(p)[1] = hi;
#else
    *p = r;
#endif
}

// One string of one read.  role as above (with P.strands == 1 only 0 and 1 occur); hist: this lane's column, word w at hist[w * hstride], zero on
// entry and zero again on return.  The patterns come from pack_task's workspace (tasks 2 * read and 2 * read + 1).  jumps_p0 counts the
// threshold jumps of role 0 alone: they are those of pml_task over the same read.
template <class XCHG>
MONI_HD void screen_task(const moni_consts_t& K, const lds_tables_t& L, const moni_row_t* __restrict__ rows, const moni_frow_t* __restrict__ frows,
                         const uint32_t* __restrict__ cr, const moni_rec_t* __restrict__ recs, const uint64_t* __restrict__ pat,
                         const uint64_t* __restrict__ offs, const moni_u64x2* __restrict__ blk, uint64_t read, uint32_t role, const moni_screen_params_t& P,
                         uint32_t* __restrict__ hist, uint32_t hstride, XCHG& X, moni_screen_res_t* __restrict__ res, unsigned long long& n_steps,
                         unsigned long long& n_jumps, unsigned long long& jumps_p0) {
    const uint32_t m = (uint32_t)(offs[read + 1] - offs[read]);
    const bool null_lane = (role & 1u) != 0;
    const uint64_t pb = ws_pat_base(blk, 2 * read + (role >> 1));
    ms_state_t S;
    S.run = (uint32_t)K.r - 1; S.pos = K.n - 1; S.abs = true; S.off = 0; S.m = m;     // start with the empty string
    S.sample = 0; S.word = 0;
    uint32_t length = 0, mx = 0, n_pos = 0, d_max = 0;
    unsigned long long jumps = 0;
    // the window that holds offset m-1 closes first: it has (m-1) % window + 1 offsets, every later one `window`
    uint32_t left = m ? (m - 1) % P.window : 0;          // steps until the current window closes
    uint32_t wlen = left + 1;
    for (uint32_t s = 0; s < m; ++s) {
        uint32_t raw;
        if (!null_lane) {                                 // P[m-1-s]: the packed bytes in the order of the steps
            if ((s & 7u) == 0) S.word = pat[pb + (uint64_t)(s >> 3) * 64u];
            raw = (uint32_t)S.word & 0xFFu;
            S.word >>= 8;
        } else {                                          // N[m-1-s] = P[s]: the byte of step t = m-1-s, the words from the other end
            const uint32_t t = m - 1 - s;
            if (s == 0 || (t & 7u) == 7u) S.word = pat[pb + (uint64_t)(t >> 3) * 64u] << (8u * (7u - (t & 7u)));
            raw = (uint32_t)(S.word >> 56);
            S.word <<= 8;
        }
        const uint32_t c = L.code[raw];
        if (c == MONI_CODE_ABSENT) {                      // n_c == 0   (spumoni.hpp:372-377)
            length = 0;
            S.pos = L.abs_pos[raw];
            S.run = L.abs_run[raw];
            S.abs = true;
        } else {
            length = pml_step(K, L, rows, frows, cr, recs, c, S, jumps) ? length + 1 : 0;
        }
        mx = length > mx ? length : mx;
        {
            const uint32_t v = length < MONI_SCREEN_BINS - 1 ? length : MONI_SCREEN_BINS - 1;
            hist[(v >> 1) * hstride] += 1u << (16u * (v & 1u));
        }
        if (left) { --left; continue; }
        // the window [m-1-s, m-1-s + wlen) closes: the columns of the pattern and the null lane into D, bins 0 .. BINS-2; both columns zero again
        // (a rolled loop: unrolled, the sixteen words in flight cost the walk its registers)
        uint32_t cum_a = 0, cum_b = 0, D = 0;
#pragma unroll 1
        for (uint32_t w = 0; w < SCREEN_WORDS; ++w) {
            const uint32_t a = hist[w * hstride];
            hist[w * hstride] = 0;
            const uint32_t b = X.pair(a);
            screen_ks_bin(a & 0xFFFFu, b & 0xFFFFu, cum_a, cum_b, D);
            if (w + 1 < SCREEN_WORDS) screen_ks_bin(a >> 16, b >> 16, cum_a, cum_b, D);
        }
        if (!null_lane && wlen >= P.min_win) {            // a scored window (a full one has window >= min_win offsets)
            d_max = D > d_max ? D : d_max;
            n_pos += D * P.ks_den >= P.ks_num * wlen ? 1u : 0u;          // both products are below 2^32
        }
        left = P.window - 1;
        wlen = P.window;
    }
    n_steps += m;
    n_jumps += jumps;
    if (role == 0) jumps_p0 += jumps;
    // strand 1's figures to the lane of strand 0, which writes the record
    uint32_t n_pos1 = 0, d_max1 = 0, mx1 = 0;
    if (P.strands == 2) { n_pos1 = X.strand(n_pos); d_max1 = X.strand(d_max); mx1 = X.strand(mx); }
    if (role == 0) {
        moni_screen_res_t R;
        R.n_win = screen_n_win(m, P);
        R.n_pos[0] = n_pos; R.n_pos[1] = n_pos1; R.d_max[0] = d_max; R.d_max[1] = d_max1; R.max_pml[0] = mx; R.max_pml[1] = mx1;
        R.flags = (R.n_win == 0 ? MONI_SCREEN_SHORT : 0u) | (2 * n_pos > R.n_win || 2 * n_pos1 > R.n_win ? MONI_SCREEN_PRESENT : 0u) |
                  (n_pos1 > n_pos ? MONI_SCREEN_STRAND1 : 0u);
        screen_store(res + read, R);
    }
}
