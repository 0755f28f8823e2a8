// Per-lane logic of the k-mismatch queries (bounded Hamming distance, substitutions only, k <= 3), host-compilable like locate_core.h (the kernels
// are in approx_kernels.hip, the host replay in tests/host_sim/approx_sim.cpp).
//
//   apx_exact   pass 1, one (pattern, strand): the exact path of loc_task, its state saved at every chunk start, the distance-0 hit
//   apx_piece   pass 2, one (task, chunk): level 0 across the chunk from its checkpoint, every subtree that leaves the exact path inside the chunk
//   apx_task_of the task of a global chunk number, over the exclusive scan of the chunk counts (the twin of sc_task_of)
//
// The search is a tree of loc_step's.  A node is (place s, interval); its own edge consumes pattern[m - 1 - s], and where the level e (the
// mismatches paid so far) is below k there is an edge for each of A / C / G / T that differs from that byte.  The walk is depth first with one saved
// state per LEVEL: the branches at a place are taken before the pattern's own byte, each runs level e + 1 from the next place to completion, then the
// level goes on.  So k + 1 states are live whatever the pattern length: level 0 and the active level in registers, the levels in between parked in
// a stack the caller provides (LDS in the kernel).  An interval that survives to place m at level e is a hit: a distinct string at distance e,
// its interval disjoint from every other hit's.
#pragma once
#include <algorithm>

#include "locate_core.h"

#define APX_STACK_WORDS 5u             // a parked level: the 4 words of its checkpoint and its place | next edge
#define APX_STACK_LEVELS 2u            // levels 1 .. k - 1 are parked (level 0 stays in registers, level k is only ever the active one)

#if defined(__HIP_DEVICE_COMPILE__)
#define APX_ADD_U64(p, v) ((void)atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)(v)))
#else
#define APX_ADD_U64(p, v) ((void)(*(p) += (v)))
#endif

// A search state in 32 bytes.  (run, off) form: w0 = lo.off << 32 | lo.run, w1 likewise for hi, w3 = 0.  Absolute form (after a general step):
// w0 = lo.pos, w1 = hi.pos, w3 = hi.run << 32 | lo.run (the guesses settle_run starts from).  w2 = toe | abs << 63.
struct alignas(32) apx_ckpt_t { uint64_t w0, w1, w2, w3; };

MONI_HD apx_ckpt_t apx_pack(const loc_state_t& S) {
    apx_ckpt_t C;
    if (S.abs) { C.w0 = S.lo.pos; C.w1 = S.hi.pos; C.w3 = (uint64_t)S.hi.run << 32 | S.lo.run; }
    else { C.w0 = (uint64_t)S.lo.off << 32 | S.lo.run; C.w1 = (uint64_t)S.hi.off << 32 | S.hi.run; C.w3 = 0; }
    C.w2 = (S.toe & ~(1ull << 63)) | (S.abs ? 1ull << 63 : 0);
    return C;
}
MONI_HD void apx_unpack(const apx_ckpt_t& C, loc_state_t& S) {
    S.abs = (C.w2 >> 63) != 0;
    S.toe = C.w2 & ~(1ull << 63);
    if (S.abs) { S.lo.pos = C.w0; S.hi.pos = C.w1; S.lo.run = (uint32_t)C.w3; S.hi.run = (uint32_t)(C.w3 >> 32); S.lo.off = S.hi.off = 0; }
    else { S.lo.pos = S.hi.pos = 0; S.lo.run = (uint32_t)C.w0; S.lo.off = (uint32_t)(C.w0 >> 32); S.hi.run = (uint32_t)C.w1; S.hi.off = (uint32_t)(C.w1 >> 32); }
}
// field by field: loc_state_t ends in padding bytes, and a copy of the whole struct between register-resident states would carry them through scratch
MONI_HD void apx_copy(loc_state_t& D, const loc_state_t& S) {
    D.lo.pos = S.lo.pos; D.lo.run = S.lo.run; D.lo.off = S.lo.off; D.hi.pos = S.hi.pos; D.hi.run = S.hi.run; D.hi.off = S.hi.off; D.toe = S.toe; D.abs = S.abs;
}
// the whole BWT: where loc_task starts
MONI_HD void apx_root(const moni_consts_t& K, loc_state_t& S) {
    S.lo.pos = 0; S.lo.run = 0; S.lo.off = 0;
    S.hi.pos = K.n - 1; S.hi.run = (uint32_t)K.r - 1; S.hi.off = MONI_OFF_END;
    S.toe = K.last_run_sample; S.abs = false;
}

// chunks of a pattern of m places (64-bit: chunk_len may be anything >= 1)
MONI_HD uint64_t apx_n_chunks(uint32_t m, uint32_t chunk_len) { return ((uint64_t)m + chunk_len - 1) / chunk_len; }

// the task of global chunk g: the last t with off[t] <= g (off: exclusive scan of the chunk counts, n_tasks + 1 entries, g < off[n_tasks])
MONI_HD uint64_t apx_task_of(const uint64_t* __restrict__ off, uint64_t n_tasks, uint64_t g) {
    uint64_t lo = 0, hi = n_tasks;
    while (hi - lo > 1) { const uint64_t mid = lo + ((hi - lo) >> 1); if (off[mid] <= g) lo = mid; else hi = mid; }
    return lo;
}

// what both passes share
struct apx_args_t {
    const moni_row_t* __restrict__ rows; const moni_frow_t* __restrict__ frows; const uint32_t* __restrict__ cr; const moni_rec_t* __restrict__ recs;
    const uint64_t* __restrict__ pat; const uint64_t* __restrict__ offs; const moni_u64x2* __restrict__ blk;
    uint32_t strands, k, max_hits, max_occ, chunk_len;
    uint64_t max_steps;                      // loc_step's of one piece; 0 = no limit
    moni_approx_res_t* __restrict__ res;     // n_tasks
    moni_approx_hit_t* __restrict__ slots;   // n_tasks * max_hits; occ_off holds the hit's toehold until the walk replaces it
};

// the byte place s consumes (pattern[m - 1 - s], strand-resolved by pack_task), through a one-word cache
struct apx_pat_t { uint64_t pb, word; uint32_t w; };
MONI_HD uint32_t apx_byte(const uint64_t* __restrict__ pat, apx_pat_t& P, uint32_t s) {
    const uint32_t w = s >> 3;
    if (w != P.w) { P.word = pat[P.pb + (uint64_t)w * 64u]; P.w = w; }
    return (uint32_t)(P.word >> (8u * (s & 7u))) & 0xFFu;
}

// A hit of task t at distance e: counted into the lane's sums, and kept where the task still has a slot.
MONI_HD void apx_hit(const apx_args_t& A, uint64_t t, uint32_t e, const loc_state_t& S, uint64_t& count) {
    const uint64_t lo = S.abs ? S.lo.pos : loc_abs(A.rows, S.lo), hi = S.abs ? S.hi.pos : loc_abs(A.rows, S.hi);
    count = hi - lo + 1;
    if (!A.max_hits) return;
    uint32_t* kept = &A.res[t].n_kept;
    if (*(volatile uint32_t*)kept >= A.max_hits) return;              // (full: the counter stops near max_hits however many hits follow)
    const uint32_t j = MONI_ATOMIC_INC_U32(kept);
    if (j >= A.max_hits) return;
    moni_approx_hit_t H;
    H.task = t; H.n_mis = e; H.n_occ = count < A.max_occ ? (uint32_t)count : A.max_occ; H.sa_lo = lo; H.count = count; H.occ_off = S.toe;
    A.slots[t * A.max_hits + j] = H;
}

// Pass 1.  ckpt (k >= 1; nullptr: none wanted): slot j > 0 of the task's chunks gets the state in front of place j * chunk_len where the exact
// path reached it; res[t].matched says how far it came, so a piece knows whether its checkpoint exists.  Writes the whole record of the task.
MONI_HD void apx_exact(const moni_consts_t& K, const lds_tables_t& L, const apx_args_t& A, uint64_t t, apx_ckpt_t* __restrict__ ckpt, loc_counts_t& N) {
    const uint64_t read = A.strands == 2 ? t >> 1 : t;
    const uint32_t strand = A.strands == 2 ? (uint32_t)t & 1u : 0u;
    const uint32_t m = (uint32_t)(A.offs[read + 1] - A.offs[read]);
    apx_pat_t P; P.pb = ws_pat_base(A.blk, 2 * read + strand); P.word = 0; P.w = 0xFFFFFFFFu;
    loc_state_t S;
    apx_root(K, S);
    moni_approx_res_t R;
    R.cnt[0] = R.cnt[1] = R.cnt[2] = R.cnt[3] = 0; R.n_hits = 0; R.hit_off = 0; R.n_kept = 0; R.complete = 1; R.matched = 0; R.reserved = 0;
    A.res[t].n_kept = 0;                                            // apx_hit takes the slot through the record in memory
    bool alive = m > 0;
    uint32_t next_ck = A.chunk_len, j = 1;                           // (a chunk_len >= m never gets there)
    for (uint32_t s = 0; s < m; ++s) {
        if (ckpt && s == next_ck) { ckpt[j++] = apx_pack(S); next_ck = s + A.chunk_len < s ? 0xFFFFFFFFu : s + A.chunk_len; }
        const uint32_t raw = apx_byte(A.pat, P, s);
        const uint32_t c = L.code[raw];
        if (raw <= 1u || c == MONI_CODE_ABSENT || !loc_step(K, L, A.rows, A.frows, A.cr, A.recs, c, S, N)) { alive = false; break; }
        ++R.matched;
    }
    if (alive) { apx_hit(A, t, 0, S, R.cnt[0]); R.n_hits = 1; R.n_kept = A.max_hits ? 1u : 0u; }
    A.res[t] = R;
}

// Pass 2.  Chunk j of task t: places [j * chunk_len, min(m, (j + 1) * chunk_len)) of level 0.  stack: APX_STACK_LEVELS * APX_STACK_WORDS words, `stride`
// apart (the kernel's [level][word][lane] in LDS).  N.steps counts every loc_step of the piece, `rewalk` those of them that repeat the exact path
// (pass 1 has counted them).  Returns false where max_steps stopped the piece.
MONI_HD bool apx_piece(const moni_consts_t& K, const lds_tables_t& L, const apx_args_t& A, uint64_t t, uint64_t j, const apx_ckpt_t* __restrict__ ckpt,
                       uint64_t* __restrict__ stack, uint32_t stride, loc_counts_t& N, unsigned long long& rewalk) {
    const uint64_t read = A.strands == 2 ? t >> 1 : t;
    const uint32_t strand = A.strands == 2 ? (uint32_t)t & 1u : 0u;
    const uint32_t m = (uint32_t)(A.offs[read + 1] - A.offs[read]);
    const uint32_t s_begin = (uint32_t)(j * A.chunk_len);
    if (A.res[t].matched < s_begin) return true;                     // the exact path died in front of this chunk: no checkpoint, nothing to branch from
    const uint32_t s_end = m - s_begin > A.chunk_len ? s_begin + A.chunk_len : m;
    apx_pat_t P; P.pb = ws_pat_base(A.blk, 2 * read + strand); P.word = 0; P.w = 0xFFFFFFFFu;
    const uint32_t ca = L.code['A'], cc = L.code['C'], cg = L.code['G'], ct = L.code['T'];
    loc_state_t S0, cur;                                             // level 0, in front of place s0
    if (j) apx_unpack(ckpt[j], S0); else apx_root(K, S0);
    apx_copy(cur, S0);                                               // the active level e, in front of place s; edge: the next to take (0..3 a letter, 4 the own byte)
    uint32_t e = 0, s = s_begin, s0 = s_begin, edge = A.k ? 0u : 4u, edge0 = edge;
    uint64_t cnt[4] = {0, 0, 0, 0}, n_hits = 0;
    const unsigned long long steps0 = N.steps;
    bool complete = true;
    while (true) {
        bool pop = false;
        if (s == (e ? m : s_end)) {                                  // the level is through: a hit above level 0, then back to the level below
            if (e) {
                uint64_t c1;
                apx_hit(A, t, e, cur, c1);
                if (e == 1) cnt[1] += c1; else if (e == 2) cnt[2] += c1; else cnt[3] += c1;
                ++n_hits;
            }
            pop = true;
        } else {
            const uint32_t raw = apx_byte(A.pat, P, s);
            const uint32_t this_edge = edge;
            uint32_t c;
            if (this_edge < 4) {                                     // a substitution: the text holds this letter where the pattern holds another byte
                ++edge;
                const uint32_t letter = this_edge == 0 ? 'A' : this_edge == 1 ? 'C' : this_edge == 2 ? 'G' : 'T';
                c = this_edge == 0 ? ca : this_edge == 1 ? cc : this_edge == 2 ? cg : ct;
                if (letter == raw || c == MONI_CODE_ABSENT) continue;
            } else c = L.code[raw];
            if (this_edge == 4 && (raw <= 1u || c == MONI_CODE_ABSENT)) pop = true;      // the level ends here; its substitutions at this place have been tried
            else {
                if (A.max_steps && N.steps - steps0 >= A.max_steps) { complete = false; break; }
                loc_state_t T;
                apx_copy(T, cur);
                const bool ok = loc_step(K, L, A.rows, A.frows, A.cr, A.recs, c, T, N);
                if (this_edge == 4) {
                    if (!e) ++rewalk;
                    if (!ok) pop = true;
                    else {
                        apx_copy(cur, T); ++s; edge = e < A.k ? 0u : 4u;
                        if (!e) { apx_copy(S0, T); s0 = s; edge0 = edge; }
                    }
                } else if (ok) {                                     // down one level: this one waits in front of the same place, its next edge noted
                    if (!e) edge0 = edge;
                    else {
                        uint64_t* q = stack + (uint64_t)(e - 1) * APX_STACK_WORDS * stride;
                        const apx_ckpt_t C = apx_pack(cur);
                        q[0] = C.w0; q[stride] = C.w1; q[2 * stride] = C.w2; q[3 * stride] = C.w3; q[4 * stride] = (uint64_t)edge << 32 | s;
                    }
                    apx_copy(cur, T); ++e; ++s; edge = e < A.k ? 0u : 4u;
                }
            }
        }
        if (pop) {
            if (!e) break;
            if (--e == 0) { apx_copy(cur, S0); s = s0; edge = edge0; }
            else {
                const uint64_t* q = stack + (uint64_t)(e - 1) * APX_STACK_WORDS * stride;
                apx_ckpt_t C; C.w0 = q[0]; C.w1 = q[stride]; C.w2 = q[2 * stride]; C.w3 = q[3 * stride];
                apx_unpack(C, cur); s = (uint32_t)q[4 * stride]; edge = (uint32_t)(q[4 * stride] >> 32);
            }
        }
    }
    moni_approx_res_t* R = A.res + t;
    if (cnt[1]) APX_ADD_U64(&R->cnt[1], cnt[1]);
    if (cnt[2]) APX_ADD_U64(&R->cnt[2], cnt[2]);
    if (cnt[3]) APX_ADD_U64(&R->cnt[3], cnt[3]);
    if (n_hits) APX_ADD_U64(&R->n_hits, n_hits);
    if (!complete) *(volatile uint32_t*)&R->complete = 0;          // (every piece that stops stores the same value)
    return complete;
}

// Host only.  The order the hit list is handed out in: grouped by task (it is), by (n_mis, sa_lo) inside one.  hits: the compact list.
inline void apx_sort_hits(moni_approx_hit_t* hits, const moni_approx_res_t* res, uint64_t n_tasks) {
    for (uint64_t t = 0; t < n_tasks; ++t)
        std::sort(hits + res[t].hit_off, hits + res[t].hit_off + res[t].n_kept,
                  [](const moni_approx_hit_t& a, const moni_approx_hit_t& b) { return a.n_mis != b.n_mis ? a.n_mis < b.n_mis : a.sa_lo < b.sa_lo; });
}
