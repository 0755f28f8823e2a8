// Per-lane code of the depth of coverage.  As bam_sort_core.h, the file compiles for the host with the lanes as loops
// (tests/host_sim/coverage_sim.cpp): every function here is what ONE lane does for one record, slot, line or window; what a wavefront does
// together (the counters' sums, the last flush of the reduce) is in cov_kernels.hip, and the host replay does it with plain sums.
//
//   cov_check     one record per lane: the record check of the sort (bam_reckey) unless the records come from it, then the record's class
//   cov_blocks    one counted record per lane: its CIGAR walked into blocks, +1 / -1 per block through `add`
//   cov_reduce    one lane's slots of the sealed array, COV_W apart: sum, minimum and maximum of the depth per reference through `flush`
//   cov_tail      one slot per lane: does a run of equal depth end here
//   cov_line      one line per lane: reference, start, end and depth of the run that ends at pos[k]; cov_line_len / cov_put_line: its text
//   cov_window    one lane's part of a window's sum
//
// The slots: reference r owns base[r] .. base[r + 1] - 1 (base has n_ref + 1 entries, base[n_ref] = S); the last of them is no base.
#pragma once
#include "bam_sort_core.h"
#include "render_core.h"

#define COV_T 256u                  // lanes of a workgroup
#define COV_W 64u                   // lanes of a wavefront
#define COV_STEPS 32u               // slots a lane takes in the reduce
#define COV_LIMIT (1ull << 31)      // counted records of one object stay below: the depth is an int32
#define COV_MAX_CALL (1ull << 30)   // slots one moni_cov_next looks at, at most: the scan of their flags is 32 bits wide

enum { COV_COUNTED = 0, COV_UNPLACED = 1, COV_FLAG = 2, COV_MAPQ = 3 };

// the class of a record whose fixed fields lie inside the buffer
BAM_FN uint32_t cov_class(const uint8_t* r, uint32_t exclude, uint32_t min_mapq) {
    const int32_t ref = (int32_t)bam_get32(r + 4), pos = (int32_t)bam_get32(r + 8);
    const uint32_t mapq = r[13], n_ops = bam_get16(r + 16), flag = bam_get16(r + 18);
    if (ref < 0 || pos < 0 || !n_ops) return COV_UNPLACED;
    if (flag & exclude) return COV_FLAG;
    if (mapq < min_mapq) return COV_MAPQ;
    return COV_COUNTED;
}

// Record i: MONI_BAMSORT_* << 8 | class.  trusted: the records left the sort of this library, which has run bam_reckey over them; only the id is
// held against this dictionary again.
BAM_FN uint32_t cov_check(const uint8_t* rec, uint64_t len, const uint64_t* off, uint64_t i, uint32_t n_ref, uint32_t exclude, uint32_t min_mapq, bool trusted) {
    if (!trusted) {
        uint64_t key; bam_pre_t pre;
        const uint32_t why = bam_reckey(rec, len, off, i, n_ref, key, pre);
        if (why) return why << 8;
    }
    const uint8_t* r = rec + off[i];
    const int32_t ref = (int32_t)bam_get32(r + 4);
    if (ref >= 0 && (uint32_t)ref >= n_ref) return (uint32_t)MONI_BAMSORT_REF << 8;
    return cov_class(r, exclude, min_mapq);
}

// A counted record at r: add(slot, +1) and add(slot, -1) for every block of its CIGAR.  M = X D cover and advance, N advances and ends the block,
// I S H P do nothing (they do not end a block either); a block without a base is none.  Returns blocks | clipped << 31.  Every slot named lies
// in [base[ref], base[ref + 1]).
template <class Add>
BAM_FN uint32_t cov_blocks(const uint8_t* r, const uint64_t* base, Add&& add) {
    const uint32_t ref = bam_get32(r + 4), l_name = r[12], n_ops = bam_get16(r + 16);
    const uint64_t b0 = base[ref], ln = base[ref + 1] - b0 - 1u;
    const uint8_t* cg = r + BAM_FIXED + l_name;
    uint64_t p = bam_get32(r + 8), bs = p;
    uint32_t nb = 0, clipped = 0;
    AFR_ROLLED for (uint32_t k = 0; k <= n_ops; ++k) {
        const uint32_t v = k < n_ops ? bam_get32(cg + 4u * (uint64_t)k) : 3u;          // behind the last operation: an N of length 0 closes the block
        const uint32_t op = v & 15u;
        if ((0x185u >> op) & 1u) { p += v >> 4; continue; }          // M D = X
        if (op != 3u) continue;
        if (p > bs) {
            if (bs >= ln) clipped = 1u;
            else {
                if (p > ln) clipped = 1u;
                add(b0 + bs, 1);
                add(b0 + (p > ln ? ln : p), -1);
                ++nb;
            }
        }
        p += v >> 4; bs = p;
    }
    return nb | clipped << 31;
}

// the reference that owns slot x < base[n_ref]
BAM_FN uint32_t cov_ref_of(const uint64_t* base, uint32_t n_ref, uint64_t x) {
    uint32_t lo = 0, hi = n_ref;          // base[lo] <= x < base[hi]
    while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (base[mid] <= x) lo = mid; else hi = mid; }
    return lo;
}
// ... from a reference r that owns a slot at or before x
BAM_FN uint32_t cov_ref_from(const uint64_t* base, uint32_t r, uint64_t x) {
    while (x >= base[r + 1u]) ++r;
    return r;
}

// what a lane has seen of one reference's depth
typedef struct { uint64_t sum; uint32_t mn, mx, ref; } cov_acc_t;
BAM_FN void cov_acc_reset(cov_acc_t& a, uint32_t ref) { a.sum = 0; a.mn = 0xFFFFFFFFu; a.mx = 0; a.ref = ref; }

// The lane's slots x0, x0 + COV_W, ... (COV_STEPS of them, those below S): flush(a) whenever the reference changes; what is left in `a` at the
// end is the caller's to flush.  An accumulator that saw no base changes nothing when flushed.
template <class Flush>
BAM_FN void cov_reduce(const int32_t* depth, const uint64_t* base, uint32_t n_ref, uint64_t S, uint64_t x0, cov_acc_t& a, Flush&& flush) {
    cov_acc_reset(a, x0 < S ? cov_ref_of(base, n_ref, x0) : n_ref - 1u);
    for (uint32_t k = 0; k < COV_STEPS; ++k) {
        const uint64_t x = x0 + (uint64_t)k * COV_W;
        if (x >= S) break;
        const uint32_t r = cov_ref_from(base, a.ref, x);
        if (r != a.ref) { flush(a); cov_acc_reset(a, r); }
        if (x + 1u == base[r + 1u]) continue;          // the reference's last slot
        const uint32_t d = (uint32_t)depth[x];
        a.sum += d; a.mn = d < a.mn ? d : a.mn; a.mx = d > a.mx ? d : a.mx;
    }
}

// Does a run end at slot x of reference r: x is a base, and the slot behind it is the reference's last or holds another depth
BAM_FN uint32_t cov_tail(const int32_t* depth, const uint64_t* base, uint32_t r, uint64_t x) {
    const uint64_t last = base[r + 1u] - 1u;
    if (x == last) return 0u;
    return (x + 1u == last || depth[x + 1u] != depth[x]) ? 1u : 0u;
}

// Line k of a call: its run ends at slot pos[k] and begins behind the run before it - behind pos[k - 1], or for the call's first line at
// `carry`, behind the last line of the calls before.  That slot may be the last of the reference before: the run then begins with its own.
typedef struct { uint32_t ref, start, end, depth; } cov_line_t;
BAM_FN cov_line_t cov_line(const int32_t* depth, const uint64_t* base, uint32_t n_ref, const uint64_t* pos, uint64_t k, uint64_t carry) {
    const uint64_t x = pos[k];
    uint64_t s = k ? pos[k - 1u] + 1u : carry;
    cov_line_t L;
    L.ref = cov_ref_of(base, n_ref, x);
    if (s < base[L.ref]) s = base[L.ref];
    L.start = (uint32_t)(s - base[L.ref]); L.end = (uint32_t)(x - base[L.ref]) + 1u; L.depth = (uint32_t)depth[x];
    return L;
}
// name \t start \t end \t depth \n
BAM_FN uint64_t cov_line_len(const cov_line_t& L, const uint32_t* name_off) {
    return (uint64_t)(name_off[L.ref + 1u] - name_off[L.ref]) + 4u + afr_ndig(L.start) + afr_ndig(L.end) + afr_ndig(L.depth);
}
BAM_FN void cov_put_line(uint8_t* dst, const cov_line_t& L, const uint8_t* names, const uint32_t* name_off) {
    const uint32_t nl = name_off[L.ref + 1u] - name_off[L.ref];
    const uint8_t* nm = names + name_off[L.ref];
    AFR_ROLLED for (uint32_t j = 0; j < nl; ++j) dst[j] = nm[j];
    dst += nl;
    const uint32_t v[3] = {L.start, L.end, L.depth};
    AFR_UNROLLED for (uint32_t f = 0; f < 3u; ++f) {
        const uint32_t nd = afr_ndig(v[f]);
        *dst++ = '\t';
        afr_put_digits(dst, v[f], nd);
        dst += nd;
    }
    *dst = '\n';
}

// a lane's part of the sum of depth[lo, hi): the slots lo + lane, lo + lane + stride, ...
BAM_FN uint64_t cov_window(const int32_t* depth, uint64_t lo, uint64_t hi, uint32_t lane, uint32_t stride) {
    uint64_t s = 0;
    for (uint64_t x = lo + lane; x < hi; x += stride) s += (uint32_t)depth[x];
    return s;
}
