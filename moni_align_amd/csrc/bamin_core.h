// Per-segment and per-record code of the BAM reader: from the inflated bytes of a BAM stream to FASTQ text.  As
// inflate_core.h, the file compiles for the host with the lanes as loops (tests/host_sim/bamin_sim.cpp): a phase is a BAMIN_LANES loop,
// BAMIN_SYNC stands between two phases, and nothing but the macros below differs between the two builds.
//
// The stream is the bytes carried over from the call before with the call's inflated bytes directly behind them; it is cut into segments
// of BAMIN_S bytes.  A record starts wherever the record before it ends (block_size is its first field), so:
//   bamin_sweep    per segment: last[p] for EVERY byte offset p, the last candidate inside the segment on the chain p -> p + 4 + le32(p)
//   bamin_header   one lane: magic, l_text, n_ref, a hop per reference
//   bamin_chain    one lane: per segment its entry (the first record start at or behind the segment's start) - one look into the table and
//                  one block_size per segment
//   bamin_list     a lane per segment: the record starts from the entry on, each record checked, into the segment's fixed slots
//   bamin_select   a lane per record: kept / secondary or supplementary / empty, the length of its FASTQ text
//   bamin_rank     paired mode, a lane per record: which mate text a kept record goes to, the flags a mate must have, the lone last one
//   bamin_fastq    a wavefront per record: the four lines
// Nothing is validated in the sweep: a wrong candidate's bytes are nobody's business.  What the chain and the list touch is a true record
// start, and every field is checked there before it is used, so no later pass leaves the stream.
#pragma once
#include "bam_sort_core.h"

#define BAMIN_S 32768u              // bytes of a segment: the table of one takes 2 * BAMIN_S = 64 KB of LDS
#define BAMIN_T 256u                // lanes of a workgroup
#define BAMIN_TILE 32u              // positions the sweep settles at a time: a live candidate points at least 36 bytes ahead
#define BAMIN_SLOTS (BAMIN_S / 36u + 1u)          // records that start inside one segment, at most
#define BAMIN_GROUP 1024u           // segments swept per launch: 32 MB of stream, 64 MB of table
#define BAMIN_MAX_BLOCK (1u << 28)
#define BAMIN_END (~0ull)           // pending: no further record start is known
#define BAMIN_NONE 0xFFFFFFFFu      // entry: no record starts in the segment;  bad: none

static_assert(BAMIN_S <= 65536u && BAMIN_S % (4u * BAMIN_T) == 0 && BAMIN_S % BAMIN_TILE == 0, "a segment's offsets are 16 bits; the phases take whole steps");
static_assert(BAMIN_TILE <= 36u, "a tile depends only on entries above its own top");

#if defined(__HIP_DEVICE_COMPILE__)
#define BAMIN_LANES(l) for (uint32_t l = threadIdx.x, once_ = 1; once_; once_ = 0)
#define BAMIN_SYNC() __syncthreads()
// between two tiles: the lanes of ONE wavefront wrote the tile, the same wavefront reads it (LDS serves a wave's requests in order)
#define BAMIN_TILE_SYNC() __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup")
#define BAMIN_TILE_WAVE() if (threadIdx.x < 64u)          // phase 2 is the first wavefront's: the others go to the barrier behind it at once
#define BAMIN_MIN64(p, v) atomicMin((p), (unsigned long long)(v))
#else
#define BAMIN_LANES(l) for (uint32_t l = 0; l < BAMIN_T; ++l)
#define BAMIN_SYNC() ((void)0)
#define BAMIN_TILE_SYNC() ((void)0)
#define BAMIN_TILE_WAVE()
#define BAMIN_MIN64(p, v) do { if ((unsigned long long)(v) < *(p)) *(p) = (unsigned long long)(v); } while (0)
#endif

// what the kernels of one call hand each other, in device memory; the host sets it before the first launch and reads it back
typedef struct {
    unsigned long long pending;     // the chain: where the next record starts, BAMIN_END when that is not known (any more)
    unsigned long long carry_off;   // everything from here on goes to the next call: the first record that is not whole, the lone first mate
    unsigned long long bad;         // the minimum of (record index since the reset << 8 | reason) over the bad records, ~0: none
    unsigned long long rec_base;    // records seen by the calls before
    unsigned long long lone_rec;    // paired mode: the record that is carried as a lone first mate, n_rec: none
    unsigned long long seen, kept, skipped_sec, skipped_empty, len1, len2;          // bamin_summary
    uint32_t header_done, pad;
} bamin_state_t;

typedef struct {
    const uint8_t* s; uint64_t n;                  // the stream
    bamin_state_t* st;
    uint16_t* table; uint64_t k0, k1;              // the group's segments [k0, k1) and their tables, BAMIN_S entries each
    uint32_t* entry; uint64_t n_seg;               // per segment of the stream
    uint32_t* slots; uint64_t* cnt; uint32_t* seg_bad; const uint64_t* pos;          // per segment: record starts, how many, (slot << 8 | reason), the scan of cnt
    uint32_t* rec_off; uint64_t n_rec;             // the records' starts, in order
    uint64_t* cls; const uint64_t* cls_x;          // per record: 1 kept, 1 << 32 secondary / supplementary, 0 empty; its scan (entry n_rec: the sums)
    uint64_t* len1; uint64_t* len2; const uint64_t* len1_x; const uint64_t* len2_x;          // bytes of text per record and mate text; their scans
    uint32_t* kept_off;                            // paired: the start of the kept record of rank j
    uint8_t* text1; uint8_t* text2;
    uint32_t paired;
} bamin_args_t;

BAM_FN void bamin_bad(bamin_state_t* st, uint64_t rec, uint32_t why) { BAMIN_MIN64(&st->bad, (st->rec_base + rec) << 8 | why); }

// bytes [a, a + 4) of the stream as a word, a a multiple of 4; bytes behind the stream's end read as zero and are not touched
BAM_FN uint32_t bamin_word(const uint8_t* s, uint64_t n, uint64_t a) {
    if (a + 4u <= n) return bam_load_word(s + a);
    uint32_t v = 0;
    for (uint32_t j = 0; j < 4u; ++j)
        if (a + j < n) v |= (uint32_t)s[a + j] << (8u * j);
    return v;
}

// ---- the sweep: segment k of the stream, by one workgroup; tbl: BAMIN_S entries of LDS; out: the segment's table in HBM -------------------
// Phase 1, all lanes: tbl[p] = where p's chain goes next inside the segment, or p itself where it ends (p is dead: its four bytes are not
// all inside the stream, or le32(p) < 32; or its next lies at or beyond the segment's end).  A lane takes four positions from two words.
// Phase 2, half a wavefront, tiles of 32 in descending order: tbl[p] = tbl[tbl[p]].  A live p has next >= p + 36, above the top of p's tile,
// where every entry already is the last of its chain.  Phase 3, all lanes: the table out, word by word.
BAM_FN void bamin_sweep(const uint8_t* s, uint64_t n, uint64_t k, uint16_t* tbl, uint16_t* out) {
    const uint64_t base = k * BAMIN_S;
    BAMIN_LANES(l) {
        for (uint32_t p = 4u * l; p < BAMIN_S; p += 4u * BAMIN_T) {
            const uint64_t a = base + p;
            const uint32_t w0 = a < n ? bamin_word(s, n, a) : 0u, w1 = a + 4u < n ? bamin_word(s, n, a + 4u) : 0u;
            for (uint32_t j = 0; j < 4u; ++j) {
                const uint32_t v = j ? bam_align_word(w0, w1, j) : w0;
                const uint64_t nx = a + j + 4u + (uint64_t)v;
                const bool ends = a + j + 4u > n || v < 32u || nx >= base + BAMIN_S;
                tbl[p + j] = (uint16_t)(ends ? p + j : (uint32_t)(nx - base));
            }
        }
    }
    BAMIN_SYNC();
    BAMIN_TILE_WAVE() for (uint32_t t = BAMIN_S / BAMIN_TILE; t-- > 0u;) {
        BAMIN_LANES(l) {
            if (l < BAMIN_TILE) {
                const uint32_t p = t * BAMIN_TILE + l, nx = tbl[p];
                if (nx != p) tbl[p] = tbl[nx];
            }
        }
        BAMIN_TILE_SYNC();
    }
    BAMIN_SYNC();
    BAMIN_LANES(l) {
        for (uint32_t q = l; q < BAMIN_S / 2u; q += BAMIN_T) {
            uint32_t v;
            __builtin_memcpy(&v, tbl + 2u * q, 4);
            __builtin_memcpy(out + 2u * q, &v, 4);
        }
    }
    BAMIN_SYNC();
}

// ---- the header, by one lane ------------------------------------------------------------------------------------------------------------------
// The stream begins with the header (all bytes are carried until it is whole).  Whole: pending = the first record's start, header_done.
// Not whole: carry_off = 0.  Bad: MONI_BAMIN_MAGIC / MONI_BAMIN_HEADER.  In the last two cases pending = BAMIN_END: no record is listed.
BAM_FN void bamin_header(const uint8_t* s, uint64_t n, bamin_state_t* st) {
    st->pending = BAMIN_END;
    for (uint32_t j = 0; j < 4u && j < n; ++j)
        if (s[j] != (uint8_t)"BAM\1"[j]) { bamin_bad(st, 0, MONI_BAMIN_MAGIC); return; }
    if (n < 12u) { st->carry_off = 0; return; }
    const int32_t l_text = (int32_t)bam_get32(s + 4);
    if (l_text < 0) { bamin_bad(st, 0, MONI_BAMIN_HEADER); return; }
    uint64_t at = 8u + (uint64_t)l_text;
    if (at + 4u > n) { st->carry_off = 0; return; }
    const int32_t n_ref = (int32_t)bam_get32(s + at);
    if (n_ref < 0) { bamin_bad(st, 0, MONI_BAMIN_HEADER); return; }
    at += 4u;
    for (int32_t r = 0; r < n_ref; ++r) {
        if (at + 4u > n) { st->carry_off = 0; return; }
        const int32_t l_name = (int32_t)bam_get32(s + at);
        if (l_name < 1) { bamin_bad(st, 0, MONI_BAMIN_HEADER); return; }
        at += 8u + (uint64_t)l_name;          // l_name, the name, l_ref
        if (at > n) { st->carry_off = 0; return; }
    }
    st->pending = at;
    st->header_done = 1u;
}

// ---- the chain over the group's segments, by one lane ----------------------------------------------------------------------------------------
// pending lies at or behind the start of segment k0 (or is BAMIN_END).  Per segment: its entry; then one look into its table - the last
// record start inside the segment - and that record's block_size give the next.  A record that is not whole or whose block_size is out of
// range ends the chain; the list finds it again and says which of the two it is.
BAM_FN void bamin_chain(const bamin_args_t& G) {
    bamin_state_t* st = G.st;
    uint64_t pending = st->pending;
    for (uint64_t k = G.k0; k < G.k1; ++k) {
        const uint64_t lo = k * BAMIN_S;
        if (pending >= lo + BAMIN_S || pending < lo) { G.entry[k] = BAMIN_NONE; continue; }          // (BAMIN_END too; below lo it never is)
        G.entry[k] = (uint32_t)pending;
        const uint64_t a = lo + G.table[(k - G.k0) * BAMIN_S + (pending - lo)];
        pending = BAMIN_END;
        if (a + 4u > G.n) continue;
        const uint32_t bs = bam_get32(G.s + a);
        if (bs < 32u || bs > BAMIN_MAX_BLOCK || a + 4u + bs > G.n) continue;
        pending = a + 4u + bs;
    }
    st->pending = pending;
}

// the checks of a record at a whose block_size bs is in range and whose bytes [a, a + 4 + bs) lie inside the stream
BAM_FN bool bamin_fields_ok(const uint8_t* r, uint32_t bs) {
    const uint32_t l_name = r[12], n_ops = bam_get16(r + 16);
    const int32_t l_seq = (int32_t)bam_get32(r + 20);
    if (l_name < 1u || l_seq < 0) return false;
    if (32u + (uint64_t)l_name + 4u * (uint64_t)n_ops + ((uint64_t)l_seq + 1u) / 2u + (uint64_t)l_seq > bs) return false;
    return r[BAM_FIXED + l_name - 1u] == 0u;
}

// ---- the list of segment k, by one lane --------------------------------------------------------------------------------------------------------
BAM_FN void bamin_list(const bamin_args_t& G, uint64_t k) {
    const uint64_t hi = k * BAMIN_S + BAMIN_S;
    uint64_t a = G.entry[k] == BAMIN_NONE ? hi : G.entry[k];
    uint32_t i = 0, bad = BAMIN_NONE;
    while (a < hi) {
        if (a + 4u > G.n) { BAMIN_MIN64(&G.st->carry_off, a); break; }
        const uint32_t bs = bam_get32(G.s + a);
        if (bs < 32u || bs > BAMIN_MAX_BLOCK) { bad = i << 8 | MONI_BAMIN_BLOCK_SIZE; break; }
        if (a + 4u + bs > G.n) { BAMIN_MIN64(&G.st->carry_off, a); break; }
        if (!bamin_fields_ok(G.s + a, bs)) { bad = i << 8 | MONI_BAMIN_FIELDS; break; }
        G.slots[k * BAMIN_SLOTS + i] = (uint32_t)a;
        i += 1u; a += 4u + bs;
    }
    G.cnt[k] = i; G.seg_bad[k] = bad;
    if (k + 1u == G.n_seg) G.cnt[G.n_seg] = 0;          // the scan's sum
}

// slot i of segment k to its place among all records; the segment's bad record gets its index (lane i == 0)
BAM_FN void bamin_compact(const bamin_args_t& G, uint64_t k, uint32_t i) {
    if (i < G.cnt[k]) G.rec_off[G.pos[k] + i] = G.slots[k * BAMIN_SLOTS + i];
    if (i == 0u && G.seg_bad[k] != BAMIN_NONE) bamin_bad(G.st, G.pos[k] + (G.seg_bad[k] >> 8), G.seg_bad[k] & 255u);
}

// ---- selection ----------------------------------------------------------------------------------------------------------------------------------
BAM_FN uint64_t bamin_text_len(const uint8_t* r) { return (uint64_t)r[12] + 2u * (uint64_t)bam_get32(r + 20) + 5u; }
BAM_FN void bamin_select(const bamin_args_t& G, uint64_t r) {
    if (r == G.n_rec) { G.cls[r] = 0; if (!G.paired) G.len1[r] = 0; return; }
    const uint8_t* rec = G.s + G.rec_off[r];
    const bool sec = (bam_get16(rec + 18) & 0x900u) != 0u, kept = !sec && bam_get32(rec + 20) != 0u;
    G.cls[r] = kept ? 1ull : sec ? 1ull << 32 : 0ull;
    if (!G.paired) G.len1[r] = kept ? bamin_text_len(rec) : 0u;
}

// paired mode: the kept records alternate first mate, second mate.  A kept record of odd count at the end is carried with all behind it.
BAM_FN void bamin_rank(const bamin_args_t& G, uint64_t r) {
    if (r == G.n_rec) { G.len1[r] = 0; G.len2[r] = 0; return; }
    const uint64_t n_kept = G.cls_x[G.n_rec] & 0xFFFFFFFFull, rank = G.cls_x[r] & 0xFFFFFFFFull;
    const bool kept = (G.cls_x[r + 1u] & 0xFFFFFFFFull) != rank;
    uint64_t l1 = 0, l2 = 0;
    if (kept) {
        const uint8_t* rec = G.s + G.rec_off[r];
        const uint32_t flag = bam_get16(rec + 18);
        G.kept_off[rank] = G.rec_off[r];
        if (!(flag & 1u) || (flag & 0xC0u) != ((rank & 1u) ? 0x80u : 0x40u)) bamin_bad(G.st, r, MONI_BAMIN_PAIRING);
        if ((n_kept & 1u) && rank + 1u == n_kept) { G.st->lone_rec = r; BAMIN_MIN64(&G.st->carry_off, G.rec_off[r]); }
        else if (rank & 1u) l2 = bamin_text_len(rec);
        else l1 = bamin_text_len(rec);
    }
    G.len1[r] = l1; G.len2[r] = l2;
}

// the figures of the call, by one lane: what lies before the lone first mate counts
BAM_FN void bamin_summary(const bamin_args_t& G) {
    bamin_state_t* st = G.st;
    const uint64_t lim = G.paired && st->lone_rec < G.n_rec ? st->lone_rec : G.n_rec;
    st->seen = lim; st->kept = G.cls_x[lim] & 0xFFFFFFFFull; st->skipped_sec = G.cls_x[lim] >> 32;
    st->skipped_empty = lim - st->kept - st->skipped_sec;
    st->len1 = G.len1_x[G.n_rec]; st->len2 = G.paired ? G.len2_x[G.n_rec] : 0u;
}

// ---- the text of record r, by one wavefront -----------------------------------------------------------------------------------------------------
BAM_FN uint32_t bamin_base(uint32_t nib) {          // =ACMGRSVTWYHKDBN with N for =
    return (uint32_t)((nib < 8u ? 0x565352474D43414Eull : 0x4E42444B48595754ull) >> (8u * (nib & 7u))) & 255u;
}
BAM_FN uint32_t bamin_compl(uint32_t nib) { return (nib & 1u) << 3 | (nib & 2u) << 1 | (nib & 4u) >> 1 | (nib & 8u) >> 3; }

// @name \n SEQ \n + \n QUAL \n; a record with 0x10 gives the read as sequenced.  Byte j of the text belongs to lane j % 64.
BAM_FN void bamin_fastq_text(const uint8_t* rec, uint8_t* out) {
    const uint32_t l_name = rec[12], n_ops = bam_get16(rec + 16), l_seq = bam_get32(rec + 20);
    const bool rev = (bam_get16(rec + 18) & 0x10u) != 0u;
    const uint8_t* seq = rec + BAM_FIXED + l_name + 4u * (uint64_t)n_ops;
    const uint8_t* qual = seq + (l_seq + 1u) / 2u;
    const bool no_qual = qual[0] == 0xFFu;
    const uint64_t b0 = (uint64_t)l_name + 1u, q0 = b0 + l_seq + 3u, size = q0 + l_seq + 1u;
    BAM_LANES(l) {
        for (uint64_t j = l; j < size; j += BAM_W) {
            uint32_t c;
            if (j < b0) c = j == 0u ? '@' : j + 1u == b0 ? '\n' : rec[BAM_FIXED + j - 1u];
            else if (j < b0 + l_seq) {
                const uint32_t i = (uint32_t)(j - b0), at = rev ? l_seq - 1u - i : i, nib = (seq[at >> 1] >> (at & 1u ? 0u : 4u)) & 15u;
                c = bamin_base(rev ? bamin_compl(nib) : nib);
            } else if (j < q0) c = j == b0 + l_seq + 1u ? '+' : '\n';
            else if (j + 1u < size) {
                const uint32_t i = (uint32_t)(j - q0);
                c = no_qual ? '"' : (uint32_t)qual[rev ? l_seq - 1u - i : i] + 33u;
            } else c = '\n';
            out[j] = (uint8_t)c;
        }
    }
}

// the name of a second mate equals that of the first (both end in NUL)
BAM_FN bool bamin_same_name(const uint8_t* a, const uint8_t* b) {
    if (a[12] != b[12]) return false;
    for (uint32_t j = 0; j < a[12]; ++j)
        if (a[BAM_FIXED + j] != b[BAM_FIXED + j]) return false;
    return true;
}

BAM_FN void bamin_fastq(const bamin_args_t& G, uint64_t r) {
    const uint8_t* rec = G.s + G.rec_off[r];
    if (G.len1_x[r + 1u] != G.len1_x[r]) { bamin_fastq_text(rec, G.text1 + G.len1_x[r]); return; }
    if (!G.paired || G.len2_x[r + 1u] == G.len2_x[r]) return;
    const uint64_t rank = G.cls_x[r] & 0xFFFFFFFFull;
    if (!bamin_same_name(G.s + G.kept_off[rank - 1u], rec)) { BAM_ONE() bamin_bad(G.st, r, MONI_BAMIN_PAIRING); }
    bamin_fastq_text(rec, G.text2 + G.len2_x[r]);
}
