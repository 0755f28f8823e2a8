// Per-record code of the coordinate sort of BAM records.  As bam_core.h, the file compiles for the host with the lanes as loops
// (tests/host_sim/bamsort_sim.cpp): what depends on the lane stands in a BAM_LANES loop or behind BAM_ONE, everything else is the same for all
// lanes of a wavefront, and nothing but those two macros differs between the two builds.
//
//   bam_reckey   one record per lane: the checks that keep every later pass inside the record, then its key and the fields of its index entry
//   bam_gather   one record per wavefront: the record's bytes from rec + off[perm[i]] to out + out_off[i], both at any byte offset
//
// The fields of a record start at any byte offset, so they are read byte by byte (bam_get16 / bam_get32).
#pragma once
#include "bam_core.h"

#define BAMSORT_T 256u              // lanes of a workgroup: 256 records in the key pass, four in the gather
#define BAMSORT_KEY_POS_BITS 33u    // (pos + 1) << 1 | reverse: pos + 1 in [0, 2^31)

// what the key pass leaves per record, in input order: the fields of the index entry that do not depend on where the record lands
typedef struct { int32_t ref_id, pos, end; uint32_t bin_flag; } bam_pre_t;

BAM_FN uint32_t bam_get16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
BAM_FN uint32_t bam_get32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// bits of the key that are sorted: 33 and the bits of n_ref (the id that unplaced records take)
BAM_FN uint32_t bam_key_bits(uint32_t n_ref) {
    uint32_t b = 0;
    while (b < 31u && (n_ref >> b)) ++b;
    return BAMSORT_KEY_POS_BITS + b;
}

// Record i of rec[0, len) with the offsets off[0, n]: MONI_BAMSORT_OK with its key and pre, or why it is a bad record.  Nothing outside
// rec[off[i], off[i + 1]) is read, and nothing of the record before its bounds are known to lie inside rec.
BAM_FN uint32_t bam_reckey(const uint8_t* rec, uint64_t len, const uint64_t* off, uint64_t i, uint32_t n_ref, uint64_t& key, bam_pre_t& pre) {
    const uint64_t a = off[i], b = off[i + 1];
    key = 0; pre.ref_id = -1; pre.pos = -1; pre.end = 0; pre.bin_flag = 0;
    if (a >= b || b > len) return MONI_BAMSORT_OFFSET;
    const uint64_t size = b - a;
    if (size < BAM_FIXED) return MONI_BAMSORT_SHORT;
    const uint8_t* r = rec + a;
    if (4u + (uint64_t)bam_get32(r) != size) return MONI_BAMSORT_SIZE;
    const int32_t ref = (int32_t)bam_get32(r + 4), pos = (int32_t)bam_get32(r + 8);
    const uint32_t l_name = r[12], bin = bam_get16(r + 14), n_ops = bam_get16(r + 16), flag = bam_get16(r + 18);
    if (size < (uint64_t)BAM_FIXED + l_name + 4u * (uint64_t)n_ops) return MONI_BAMSORT_SHORT;
    if (l_name < 1u) return MONI_BAMSORT_NAME;
    if (ref < -1 || (ref >= 0 && (uint32_t)ref >= n_ref)) return MONI_BAMSORT_REF;
    if (pos < -1 || pos >= 0x7FFFFFFF) return MONI_BAMSORT_POS;
    uint64_t reflen = 0;
    const uint8_t* cg = r + BAM_FIXED + l_name;
    for (uint32_t k = 0; k < n_ops; ++k) {
        const uint32_t v = bam_get32(cg + 4u * (uint64_t)k);
        if ((0x18Du >> (v & 15u)) & 1u) reflen += v >> 4;          // M D N = X, as bam_line has it
    }
    int64_t end = (int64_t)pos + (int64_t)(reflen ? reflen : 1u);
    if (end > 0x7FFFFFFFll) end = 0x7FFFFFFFll;          // an int32 field: a CIGAR that runs past 2^31 - 1 ends there
    const uint64_t tid = ref < 0 ? (uint64_t)n_ref : (uint64_t)ref;
    key = tid << BAMSORT_KEY_POS_BITS | (uint64_t)(uint32_t)(pos + 1) << 1 | (uint64_t)(flag >> 4 & 1u);
    pre.ref_id = ref; pre.pos = pos; pre.end = (int32_t)end; pre.bin_flag = bin << 16 | flag;
    return MONI_BAMSORT_OK;
}

// a 4-byte word at an address that is a multiple of 4
BAM_FN uint32_t bam_load_word(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, __builtin_assume_aligned(p, 4), 4);
    return v;
}
BAM_FN void bam_store_word(uint8_t* p, uint32_t v) { __builtin_memcpy(__builtin_assume_aligned(p, 4), &v, 4); }

// bytes sh .. sh + 3 of the eight bytes lo, hi (little endian), sh in 1..3
BAM_FN uint32_t bam_align_word(uint32_t lo, uint32_t hi, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
    return lo >> (8u * sh) | hi << (32u - 8u * sh);
#endif
}

// n bytes from src to dst, by one wavefront.  The head (up to the first multiple of 4 of dst) and the tail go byte by byte; the words between
// are whole words of dst, each put together from the two aligned words of src that hold its bytes - or copied, where src and dst have the same
// phase.  A word of dst belongs to the middle only while the second of its source words still lies inside [src, src + n): no byte outside the
// record is read behind it, and before it only the bytes that share an aligned word with its first (the buffer begins at a multiple of 4).
// Every byte of dst is written once, by one lane.
BAM_FN void bam_gather(const uint8_t* src, uint8_t* dst, uint64_t n) {
    const uint64_t head = ((uint64_t)0 - (uint64_t)(uintptr_t)dst) & 3u;
    if (n < head + 8u) {
        BAM_LANES(l) {
            for (uint64_t j = l; j < n; j += BAM_W) dst[j] = src[j];
        }
        return;
    }
    const uint32_t sh = (uint32_t)((uintptr_t)(src + head) & 3u);
    const uint8_t* s0 = src + head - sh;          // the aligned word that holds the first byte of the middle
    // word w of the middle reads s0[4w, 4w + 8) when sh != 0 (up to src + head - sh + 4w + 8 <= src + n) and s0[4w, 4w + 4) when it is 0
    const uint64_t words = sh ? (n - head + sh - 4u) / 4u : (n - head) / 4u;
    const uint64_t tail = head + 4u * words;
    BAM_LANES(l) {
        if (l < head) dst[l] = src[l];
        for (uint64_t w = l; w < words; w += BAM_W) {
            const uint32_t lo = bam_load_word(s0 + 4u * w);
            bam_store_word(dst + head + 4u * w, sh ? bam_align_word(lo, bam_load_word(s0 + 4u * w + 4u), sh) : lo);
        }
        for (uint64_t j = tail + l; j < n; j += BAM_W) dst[j] = src[j];
    }
}
