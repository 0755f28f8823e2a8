// Per-record and per-entry code of duplicate marking.  As bam_sort_core.h, the file compiles for the host with the lanes as
// loops (tests/host_sim/markdup_sim.cpp): what depends on the lane stands in a BAM_LANES loop or behind BAM_ONE, and only bam_wave_sum differs
// between the two builds.
//
//   bam_dupsig     one record per wavefront: the SEQ check, the score (the lanes stride the qualities), the unclipped 5' end and the end code
//   bam_dupunit    one unit per lane (a pair of adjacent records, or one record): the MATE checks and the unit's entries, none to two
//   bam_dupprep    one entry per lane: its run, the places of its records among all marks, the keys of the first sort passes
//   bam_duppair / bam_dupend   one sorted element per lane: is it a duplicate
//   bam_setdup     one record per lane: 0x400 into the flag of a marked record
//
// Every function runs on records that bam_reckey has passed: the fixed fields, the name and the CIGAR lie inside the record.
#pragma once
#include "bam_sort_core.h"

#define BAMDUP_PART 1u        // bits of a signature: the record takes part (mapped, primary)
#define BAMDUP_MULTI 2u       // flag & 1
#define BAMDUP_R1 4u          // flag & 0x40
#define BAMDUP_R2 8u          // flag & 0x80
#define BAMDUP_MAX_SCORE 0x7FFFFFFFu          // a record's score saturates here, so a pair's fits 32 bits
#define BAMDUP_NONE 0xFFFFFFFFu

typedef struct { uint64_t e; uint32_t score, bits; } bam_dupsig_t;

// the sum of v over the lanes of the wavefront (the host build has one accumulator for all lanes)
BAM_FN uint64_t bam_wave_sum(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((long long)v, o);
#endif
    return v;
}

// bits of an end code that are sorted: 34 and the bits of n_ref (the id that records without a reference take)
BAM_FN uint32_t bam_dup_bits(uint32_t n_ref) {
    uint32_t b = 0;
    while (b < 30u && (n_ref >> b)) ++b;
    return 34u + b;
}

// Record r[0, size), by one wavefront.  MONI_BAMSORT_OK with its signature, or SEQ / CLIP.
BAM_FN uint32_t bam_dupsig(const uint8_t* r, uint64_t size, uint32_t n_ref, bam_dupsig_t& s) {
    const int32_t ref = (int32_t)bam_get32(r + 4), pos = (int32_t)bam_get32(r + 8);
    const uint32_t l_name = r[12], n_ops = bam_get16(r + 16), flag = bam_get16(r + 18), l_seq = bam_get32(r + 20);
    s.e = 0; s.score = 0;
    s.bits = (flag & 1u ? BAMDUP_MULTI : 0u) | (flag & 0x40u ? BAMDUP_R1 : 0u) | (flag & 0x80u ? BAMDUP_R2 : 0u);
    const uint64_t qual = (uint64_t)BAM_FIXED + l_name + 4u * (uint64_t)n_ops + ((uint64_t)l_seq + 1u) / 2u;
    if (size < qual + l_seq) return MONI_BAMSORT_SEQ;          // before anything reads the qualities
    if (flag & 0x904u) return MONI_BAMSORT_OK;                 // unmapped, secondary or supplementary: no entry
    uint64_t part = 0;
    BAM_LANES(l) {
        for (uint64_t j = l; j < l_seq; j += BAM_W) {
            const uint32_t q = r[qual + j];
            if (q >= 15u && q != 0xFFu) part += q;
        }
    }
    const uint64_t sum = bam_wave_sum(part);
    // the clips: S and H ops before the first other op and behind the last; the reference length as bam_reckey has it, not raised to 1
    const uint8_t* cg = r + BAM_FIXED + l_name;
    uint64_t lead = 0, trail = 0, reflen = 0;
    uint32_t a = 0, b = n_ops;
    for (; a < n_ops; ++a) {
        const uint32_t v = bam_get32(cg + 4u * (uint64_t)a);
        if ((v & 15u) != 4u && (v & 15u) != 5u) break;
        lead += v >> 4;
    }
    for (; b > a; --b) {
        const uint32_t v = bam_get32(cg + 4u * (uint64_t)(b - 1u));
        if ((v & 15u) != 4u && (v & 15u) != 5u) break;
        trail += v >> 4;
    }
    for (uint32_t k = a; k < b; ++k) {
        const uint32_t v = bam_get32(cg + 4u * (uint64_t)k);
        if ((0x18Du >> (v & 15u)) & 1u) reflen += v >> 4;
    }
    const uint32_t rev = flag >> 4 & 1u;
    const int64_t u5 = rev ? (int64_t)pos + (int64_t)reflen - 1 + (int64_t)trail : (int64_t)pos - (int64_t)lead;
    if (u5 < -(1ll << 31) || u5 >= 3ll << 31) return MONI_BAMSORT_CLIP;
    const uint64_t tid = ref < 0 ? (uint64_t)n_ref : (uint64_t)ref;
    s.e = tid << 34 | (uint64_t)(u5 + (1ll << 31)) << 1 | rev;
    s.score = sum > BAMDUP_MAX_SCORE ? BAMDUP_MAX_SCORE : (uint32_t)sum;
    s.bits |= BAMDUP_PART;
    return MONI_BAMSORT_OK;
}

// do records i and j carry the same name
BAM_FN bool bam_same_name(const uint8_t* rec, const uint64_t* off, uint64_t i, uint64_t j) {
    const uint8_t* x = rec + off[i];
    const uint8_t* y = rec + off[j];
    const uint32_t n = x[12];
    if (y[12] != n) return false;
    for (uint32_t k = 0; k < n; ++k)
        if (x[BAM_FIXED + k] != y[BAM_FIXED + k]) return false;
    return true;
}

BAM_FN void bam_dup_fragment(const bam_dupsig_t& s, uint32_t at, moni_bam_dup_t& d) {
    d.k1 = s.e; d.k2 = 0; d.score = s.score; d.kind = 0; d.idx[0] = at; d.idx[1] = BAMDUP_NONE;
}

// Unit u of n records: records 2u and 2u + 1 with `paired`, record u without.  where[r]: the place of record r in the sorted run.  Returns
// MONI_BAMSORT_OK with the unit's entries - d0 where has0 (the pair, or the first record's fragment), d1 where has1 (the second record's
// fragment); in the list d0 comes first -, or MONI_BAMSORT_MATE with `bad` the unit's first record.
BAM_FN uint32_t bam_dupunit(const uint8_t* rec, const uint64_t* off, const bam_dupsig_t* sig, const uint32_t* where, uint64_t n, uint64_t u, uint32_t paired,
                            uint32_t& has0, moni_bam_dup_t& d0, uint32_t& has1, moni_bam_dup_t& d1, uint64_t& bad) {
    has0 = has1 = 0;
    if (!paired) {
        if (sig[u].bits & BAMDUP_PART) { bam_dup_fragment(sig[u], where[u], d0); has0 = 1; }
        return MONI_BAMSORT_OK;
    }
    const uint64_t i = 2u * u, j = i + 1u;
    bad = i;
    if (j >= n) return MONI_BAMSORT_MATE;          // an odd number of records
    const bam_dupsig_t& s1 = sig[i];
    const bam_dupsig_t& s2 = sig[j];
    // a record with flag & 1 carries its read's bit and not the other's; one without (the aligner writes an unaligned pair as two records of flag 4) is not asked
    const uint32_t rd = BAMDUP_R1 | BAMDUP_R2;
    if (((s1.bits & BAMDUP_MULTI) && (s1.bits & rd) != BAMDUP_R1) || ((s2.bits & BAMDUP_MULTI) && (s2.bits & rd) != BAMDUP_R2) || !bam_same_name(rec, off, i, j))
        return MONI_BAMSORT_MATE;
    const uint32_t both = BAMDUP_PART | BAMDUP_MULTI;
    if ((s1.bits & both) == both && (s2.bits & both) == both) {
        const bool lo1 = s1.e <= s2.e;          // at a tie read 1
        d0.k1 = lo1 ? s1.e : s2.e; d0.k2 = lo1 ? s2.e : s1.e;
        d0.score = s1.score + s2.score;
        d0.kind = ((s1.e ^ s2.e) & 1u) == 0 && !lo1 ? 3u : 1u;
        d0.idx[0] = where[i]; d0.idx[1] = where[j];
        has0 = 1;
        return MONI_BAMSORT_OK;
    }
    bam_dup_fragment(s1, where[i], d0); has0 = s1.bits & BAMDUP_PART ? 1u : 0u;          // both written whatever has0 and has1 say: no store through a chosen pointer
    bam_dup_fragment(s2, where[j], d1); has1 = s2.bits & BAMDUP_PART ? 1u : 0u;
    return MONI_BAMSORT_OK;
}

// ---- the resolve: all entries of all runs, one behind the other ------------------------------------------------------------------------------
// ent_base[0, n_runs]: where a run's entries begin among all entries; rec_base[0, n_runs]: where its marks begin among all marks.
// Entry j: its records' places among all marks in at[2j], at[2j + 1] (BAMDUP_NONE: none), the first key of the pair passes in pkey[j], and its
// two end slots 2j, 2j + 1 with their first keys in ekey.  A first key is class << 32 | ~score: descending scores within a class.
// The classes of an end: 0 an end of a pair, 1 a fragment, 2 the empty second slot of a fragment.  false: an idx outside its run.
BAM_FN bool bam_dupprep(const moni_bam_dup_t* ent, const uint64_t* ent_base, const uint64_t* rec_base, uint64_t n_runs, uint64_t j, uint32_t* at,
                        uint64_t* pkey, uint64_t* ekey) {
    uint64_t lo = 0, hi = n_runs;          // the last run that begins at or before j
    while (hi - lo > 1u) {
        const uint64_t mid = (lo + hi) / 2u;
        if (ent_base[mid] <= j) lo = mid; else hi = mid;
    }
    const moni_bam_dup_t d = ent[j];
    const uint64_t n_rec = rec_base[lo + 1u] - rec_base[lo];
    const bool frag = d.kind == 0;
    const bool ok = d.idx[0] < n_rec && (frag ? d.idx[1] == BAMDUP_NONE : d.idx[1] < n_rec) && (d.kind == 0 || d.kind == 1u || d.kind == 3u);
    at[2u * j] = ok ? (uint32_t)(rec_base[lo] + d.idx[0]) : BAMDUP_NONE;
    at[2u * j + 1u] = ok && !frag ? (uint32_t)(rec_base[lo] + d.idx[1]) : BAMDUP_NONE;
    const uint64_t inv = (uint64_t)(0xFFFFFFFFu - d.score);
    pkey[j] = (uint64_t)d.kind << 32 | inv;
    ekey[2u * j] = (uint64_t)(frag ? 1u : 0u) << 32 | inv;
    ekey[2u * j + 1u] = (uint64_t)(frag ? 2u : 0u) << 32 | inv;
    return ok;
}

// the end code of slot s
BAM_FN uint64_t bam_dup_end(const moni_bam_dup_t* ent, uint32_t s) { return s & 1u ? (ent[s >> 1].kind ? ent[s >> 1].k2 : ~0ull) : ent[s >> 1].k1; }

// place i of the pairs' order (perm: by k1, k2, kind, score descending, ordinal): a pair that equals its predecessor's (k1, k2, kind)
BAM_FN bool bam_duppair(const moni_bam_dup_t* ent, const uint32_t* perm, uint64_t i) {
    const moni_bam_dup_t d = ent[perm[i]];
    if (!d.kind || !i) return false;
    const moni_bam_dup_t p = ent[perm[i - 1u]];
    return p.k1 == d.k1 && p.k2 == d.k2 && p.kind == d.kind;
}

// place i of the ends' order (perm: by e, class, score descending, ordinal): a fragment that is not the first of its group
BAM_FN bool bam_dupend(const moni_bam_dup_t* ent, const uint32_t* perm, uint64_t i) {
    const uint32_t s = perm[i];
    if ((s & 1u) || ent[s >> 1].kind || !i) return false;
    return bam_dup_end(ent, perm[i - 1u]) == ent[s >> 1].k1;
}

// record i of rec[0, len), marked: the high byte of its flag, where the whole fixed part lies inside rec (bam_reckey judges the record afterwards)
BAM_FN void bam_setdup(uint8_t* rec, uint64_t len, const uint64_t* off, uint64_t i, const uint8_t* marks) {
    if (!marks[i]) return;
    const uint64_t a = off[i];
    if (a <= len && len - a >= BAM_FIXED) rec[a + 19u] |= 0x04u;
}
