// Per-lane logic of matching statistics of long patterns (moni_ms_long_batch; the legacy `moni ms` / `moni mems` with a chromosome as the pattern):
// host-compilable like seed_core.h (the kernels are in mslong_kernels.hip, the host replay in tests/host_sim/mslong_sim.cpp).
//
//   mslong_walk    ms_pointers::_query            include/ms/moni.hpp:568-624, one SEGMENT of a pattern per lane
//   mslong_len     the length loop of both legacy front ends   src/matching_statistics.cpp:242-256, src/mems.cpp:241-258
//
// The walk of ms_task is sequential along a pattern: one lane, one dependent row fetch per base.  Here a pattern is cut into segments [a, b) and
// every segment is walked by a lane of its own, which begins with the empty string at e = min(b + overlap, m), `overlap` bases to the right of
// its segment, and keeps what it computes for [a, b) (mslong_walk).  Such a walk computes the matching statistics of the truncated pattern
// P[..e).  The length pass (mslong_len) measures the match at every pointer against the text: where (b - 1) + l[b - 1] < e the truncation cannot
// have been seen and pointers and lengths of the segment are those of the whole pattern; otherwise the segment is flagged.  A maximal run of
// flagged segments is walked again by ONE lane that continues from the state the accepted segment to its right saved at its first base
// (mslong_walk with a start state), and measured again (DESIGN.md 7.7 has the proof).
//
// Consequences: lengths are the matching statistics (unique: identical to moni_ms_lengths_batch and to the reference).  Pointers are valid -
// the text at pointers[i] agrees with the pattern at i over lengths[i] bases - but where a pattern was cut they need not be the positions the
// reference reports: any position with a maximal match qualifies.  With seg_len >= the longest pattern nothing is cut and the walk is the
// reference's, pointers included.
//
// ms_step and the row accessors are seed_core.h's, unchanged.  Pattern bytes are read where moni_reads_upload-style uploads put them (the batch's
// bytes, 8-byte aligned and padded), eight per load; no packed workspace, no second strand.
#pragma once
#include "seed_core.h"

struct mslong_seg_t { uint32_t pat, a, b, e; };                          // pattern, [a, b) and where its speculative walk begins
struct alignas(8) mslong_state_t { uint64_t pos, sample; uint32_t run, off; };      // the walk's state at a segment's first base; off == MSLONG_OFF_ABS: pos is absolute (ms_state_t::abs)
#define MSLONG_OFF_ABS 0xFFFFFFFEu          // (an absolute state's off is not read: ms_step takes it from pos)
struct mslong_run_t { uint32_t s0, s1; };                                // a maximal run of flagged segments s0 .. s1 (of one pattern)

// The cuts of a pattern of m bases whose first output index is g0.  seg_len is taken down to a multiple of 8 (sl8) and the first segment shortened
// so that every later segment begins at a multiple of 8 of the OUTPUT index: groups of 8 pointers (64 bytes) and of 4 lengths (16 bytes) then
// lie inside one segment.  A pattern of at most seg_len bases is one segment, an empty pattern none.
MONI_HD uint32_t mslong_first_len(uint64_t g0, uint32_t seg_len) { return (seg_len & ~7u) - (uint32_t)(g0 & 7u); }
MONI_HD uint64_t mslong_n_segs(uint64_t g0, uint64_t m, uint32_t seg_len) {
    if (m == 0) return 0;
    if (m <= seg_len) return 1;
    const uint64_t f = mslong_first_len(g0, seg_len), sl8 = seg_len & ~7u;
    return 1 + (m - f + sl8 - 1) / sl8;
}
MONI_HD mslong_seg_t mslong_seg(uint32_t pat, uint64_t g0, uint64_t m, uint32_t seg_len, uint32_t overlap, uint64_t j) {
    mslong_seg_t s; s.pat = pat;
    uint64_t a = 0, b = m;
    if (m > seg_len) {
        const uint64_t f = mslong_first_len(g0, seg_len), sl8 = seg_len & ~7u;
        a = j ? f + (j - 1) * sl8 : 0;
        b = f + j * sl8 < m ? f + j * sl8 : m;
    }
    const uint64_t e = b + overlap < m ? b + overlap : m;
    s.a = (uint32_t)a; s.b = (uint32_t)b; s.e = (uint32_t)e;
    return s;
}

// The pointers of one aligned group of 8 output places wait here until the group is complete: place j's low word at lo[j * stride], bits 32..39
// at hi[j * stride], sign-extended when read.  A sample is a text position (below 2^39: moni_ms_long_batch refuses a longer text) or, after a byte
// the BWT does not hold set it to 0 and matches went on, 0 minus the number of those matches, as the reference's unsigned arithmetic leaves it
// (moni.hpp:583-594) - fewer than 2^32, so 40 bits with the sign say which.  In the kernels this is LDS, [place][lane] (10 KB per block of 256 lanes); kept in registers the
// group costs 10 - 16 of them and mslong_walk_kernel no longer fits 64 (8 waves per SIMD) without scratch.
struct mslong_grp_t { uint32_t* lo; uint8_t* hi; uint32_t stride; };

// eight pointers to p (on the device p is 64-byte aligned: four 16-byte stores into one line)
MONI_HD void mslong_store8(uint64_t* __restrict__ p, uint64_t q0, uint64_t q1, uint64_t q2, uint64_t q3, uint64_t q4, uint64_t q5, uint64_t q6, uint64_t q7) {
#if defined(__HIP_DEVICE_COMPILE__)
    moni_u64x2* __restrict__ v = reinterpret_cast<moni_u64x2*>(p);
    moni_u64x2 t;
    t.x = q0; t.y = q1; v[0] = t;
    t.x = q2; t.y = q3; v[1] = t;
    t.x = q4; t.y = q5; v[2] = t;
    t.x = q6; t.y = q7; v[3] = t;
#else
    p[0] = q0; p[1] = q1; p[2] = q2; p[3] = q3; p[4] = q4; p[5] = q5; p[6] = q6; p[7] = q7;
#endif
}

// One walk from pattern position `from` - 1 down to `a`, writing the pointers of [a, b) (b <= from) to ptr[g0 + k]: ptr is the plain array in
// pattern order.  start == nullptr: begin with the empty string (ms_task's start; the speculative walk, from = e); otherwise continue from
// *start, the state some walk saved at position `from` (the chain re-walk, from = b).  save (may be nullptr) receives the state at a.
// seq: the batch's bytes, 8-byte aligned; off: the pattern's first byte in it.  G: the lane's group buffer.
MONI_HD void mslong_walk(const moni_consts_t& K, const lds_tables_t& L, const moni_row_t* __restrict__ rows, const moni_frow_t* __restrict__ frows,
                         const uint32_t* __restrict__ cr, const moni_rec_t* __restrict__ recs, const uint8_t* __restrict__ seq, uint64_t off, uint64_t g0,
                         uint32_t a, uint32_t b, uint32_t from, const mslong_state_t* __restrict__ start, uint64_t* __restrict__ ptr,
                         mslong_state_t* __restrict__ save, const mslong_grp_t G, unsigned long long& n_steps, unsigned long long& n_jumps) {
    ms_state_t S;
    S.word = 0; S.m = 0;
    if (start) {
        const mslong_state_t st = *start;
        S.pos = st.pos; S.sample = st.sample; S.run = st.run; S.off = st.off; S.abs = st.off == MSLONG_OFF_ABS;
    } else {
        S.run = (uint32_t)K.r - 1; S.pos = K.n - 1; S.abs = true; S.off = 0; S.sample = K.last_run_sample;      // the empty string (seed_core.h: ms_task)
    }
    uint64_t* __restrict__ out = ptr + g0;
    const uint8_t* __restrict__ pb = seq + off;
    const uint32_t g7 = (uint32_t)g0 & 7u;
#define MSL_Q(j) ((uint64_t)G.lo[(j) * G.stride] | ((uint64_t)(int64_t)(int8_t)G.hi[(j) * G.stride] << 32))
    uint64_t word = 0;
    bool have = false;
    for (uint32_t k = from; k-- > a;) {
        const uint8_t* at = pb + k;                           // the pattern's byte k: one aligned 8-byte load serves 8 steps
        const uint32_t a7 = (uint32_t)(uintptr_t)at & 7u;
        if (!have || a7 == 7u) { word = *reinterpret_cast<const uint64_t*>(at - a7); have = true; }
        const uint32_t raw = (uint32_t)(word >> (8u * a7)) & 0xFFu;
        const uint32_t c = L.code[raw];
        if (c == MONI_CODE_ABSENT) {                          // n_c == 0   (moni.hpp:583-588)
            S.sample = 0;
            S.pos = L.abs_pos[raw];
            S.run = L.abs_run[raw];
            S.abs = true;
        } else {
            ms_step(K, L, rows, frows, cr, recs, c, S, n_jumps);
        }
        if (k >= b) continue;                                 // the overlap: walked, not written
        const uint32_t sl = (g7 + k) & 7u;
        G.lo[sl * G.stride] = (uint32_t)S.sample; G.hi[sl * G.stride] = (uint8_t)(S.sample >> 32);
        if (sl == 0) {
            if (b - k >= 8u) mslong_store8(out + k, MSL_Q(0), MSL_Q(1), MSL_Q(2), MSL_Q(3), MSL_Q(4), MSL_Q(5), MSL_Q(6), MSL_Q(7));
            else {                                            // the group runs past b: value by value
                const uint32_t nv = b - k;
                out[k] = MSL_Q(0); if (nv > 1) out[k + 1] = MSL_Q(1); if (nv > 2) out[k + 2] = MSL_Q(2); if (nv > 3) out[k + 3] = MSL_Q(3);
                if (nv > 4) out[k + 4] = MSL_Q(4); if (nv > 5) out[k + 5] = MSL_Q(5); if (nv > 6) out[k + 6] = MSL_Q(6);
            }
        }
    }
    {   // the group that holds position a begins in front of it: its values were not stored above
        const uint32_t r = (g7 + a) & 7u;
        if (r && b > a) {
            const uint32_t nv = b - a;                        // places r .. 7 of the group hold positions a .. a + 7 - r
            if (r <= 1 && nv > 1 - r) out[a + 1 - r] = MSL_Q(1);
            if (r <= 2 && nv > 2 - r) out[a + 2 - r] = MSL_Q(2);
            if (r <= 3 && nv > 3 - r) out[a + 3 - r] = MSL_Q(3);
            if (r <= 4 && nv > 4 - r) out[a + 4 - r] = MSL_Q(4);
            if (r <= 5 && nv > 5 - r) out[a + 5 - r] = MSL_Q(5);
            if (r <= 6 && nv > 6 - r) out[a + 6 - r] = MSL_Q(6);
            if (nv > 7 - r) out[a + 7 - r] = MSL_Q(7);
        }
    }
#undef MSL_Q
    if (save) {
        mslong_state_t st;
        st.pos = S.pos; st.sample = S.sample; st.run = S.run; st.off = S.abs ? MSLONG_OFF_ABS : S.off;
        *save = st;
    }
    n_steps += from - a;
}

// four lengths to p (16-byte aligned on the device: one store), as pml_core.h's pml_store4
MONI_HD void mslong_store4(uint32_t* __restrict__ p, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
#if defined(__HIP_DEVICE_COMPILE__)
    moni_u64x2 v; v.x = (uint64_t)a | ((uint64_t)b << 32); v.y = (uint64_t)c | ((uint64_t)d << 32);
    *reinterpret_cast<moni_u64x2*>(p) = v;
#else
    p[0] = a; p[1] = b; p[2] = c; p[3] = d;
#endif
}

// The length loop of the legacy front ends over positions [a, b) of a pattern of m bases, beginning with l = 0 and no previous pointer:
// lens[g0 + i] = the bases the text at ptr[g0 + i] shares with the pattern at i, compared up to pattern position `lim` (a <= b <= lim <= m).
// Returns (b - 1) + l[b - 1], the largest pattern position a comparison of [a, b) reached (i + l[i] never decreases along the loop).
//   round 1 (one lane per segment, lim = e): the segment is flagged iff the return value is >= e and e < m.  A comparison that stops at e
//     instead of m changes no verdict and no accepted length - l is min(what the bound m gives, e - i) at every i - and keeps the round's work
//     linear when a pattern is a substring of the text.
//   round 2 (one lane per run of flagged segments, after the chain re-walk, lim = m): the lengths are final.
// Pointers that are no text position (>= n: the walk went on matching after a byte the BWT does not hold, see mslong_grp_t) cannot be compared; the
// reference's loop leaves such a place the length it carries from its left neighbour.  Beginning with l = 0 at such a place would differ, so a
// range that begins with them (a > 0) leaves them to the lane on its left, and every lane goes on beyond b while they last.  They are the same
// in every walk - the byte resets the state - so no round changes whose they are.
MONI_HD uint64_t mslong_len(const moni_consts_t& K, const uint8_t* __restrict__ text, const uint8_t* __restrict__ seq, uint64_t off, uint64_t g0,
                            uint32_t a, uint32_t b, uint32_t lim, uint32_t m, const uint64_t* __restrict__ ptr, uint32_t* __restrict__ lens) {
    const uint64_t n = K.n_text;
    uint64_t l = 0, prev_pos_plus_one = n + 1;
    text_cache_t tc; tc.w = ~0ull; tc.word = 0;
    text_cache_t pc; pc.w = ~0ull; pc.word = 0;               // the pattern's bytes through the same one-word cache
    uint32_t q0 = 0, q1 = 0, q2 = 0, q3 = 0;                  // the lengths of one aligned group of 4 output places
    const uint64_t* __restrict__ pin = ptr + g0;
    uint32_t* __restrict__ out = lens + g0;
    if (a > 0) while (a < b && pin[a] >= K.n) ++a;            // the left neighbour's
    uint64_t reach = 0;
    for (uint32_t i = a; i < b; ++i) {
        const uint64_t pos = pin[i];
        while (pos != prev_pos_plus_one && (i + l) < lim && (pos + l) < n) {
            if (text_byte(seq, off + i + l, pc) != text_byte(text, pos + l, tc)) break;
            ++l;
        }
        const uint32_t sl = (uint32_t)(g0 + i) & 3u;
        if (sl == 0) q0 = (uint32_t)l; else if (sl == 1) q1 = (uint32_t)l; else if (sl == 2) q2 = (uint32_t)l; else q3 = (uint32_t)l;
        if (sl == 3 || i + 1 == b) {
            if (sl == 3 && i - a >= 3u) mslong_store4(out + (i - 3u), q0, q1, q2, q3);
            else {                                            // a group that a neighbouring segment or pattern shares: value by value
                const uint32_t nv = i - a < sl ? i - a + 1u : sl + 1u;          // places sl + 1 - nv .. sl hold positions i + 1 - nv .. i
                out[i] = sl == 0 ? q0 : sl == 1 ? q1 : sl == 2 ? q2 : q3;
                if (nv > 1) out[i - 1] = sl == 1 ? q0 : sl == 2 ? q1 : q2;
                if (nv > 2) out[i - 2] = sl == 2 ? q0 : q1;
                if (nv > 3) out[i - 3] = q0;
            }
        }
        if (i + 1 == b) reach = (uint64_t)i + l;
        l = (l == 0 ? 0 : (l - 1));
        prev_pos_plus_one = pos + 1;
    }
    if (a < b)                                                // the places behind b that no lane of their own takes
        for (uint32_t i = b; i < m && pin[i] >= K.n; ++i) {
            const uint64_t pos = pin[i];
            while (pos != prev_pos_plus_one && (i + l) < m && (pos + l) < n) {
                if (text_byte(seq, off + i + l, pc) != text_byte(text, pos + l, tc)) break;
                ++l;
            }
            out[i] = (uint32_t)l;
            l = (l == 0 ? 0 : (l - 1));
            prev_pos_plus_one = pos + 1;
        }
    return reach;
}
