// render_core.h: what one lane of finish_render_kernel does for one piece of a SAM line, in functions that also compile for the host
// (tests/host_sim/render_sim.cpp assembles lines lane by lane from them and compares with snprintf).  A line (sam.hpp:144-188) is a list
// of SEGMENTS: segments 0 .. 34 are the fixed skeleton of an aligned record, six more follow per alternative, the newline closes the list.
// Segment i of the skeleton is lane i's for the whole kernel: its entry of afr_tab says what it is and which word of the recipe's header
// it prints; the handful of things that vary per read (unmapped: "*" in place of RNAME and CIGAR; no qualities: "*"; ZS only when
// score2 != 0; the strand's "," "+" ",") are selects on that entry, the same few instructions for every lane.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AFR_HD __host__ __device__ __forceinline__
#else
#define AFR_HD inline
#endif
#if defined(__clang__)
#define AFR_ROLLED _Pragma("clang loop unroll(disable)")          // loops whose trip counts differ between lanes: unrolling them only adds registers
#define AFR_UNROLLED _Pragma("clang loop unroll(full)")
#else
#define AFR_ROLLED
#define AFR_UNROLLED
#endif

// every literal of a line, and the tables of CIGAR letters and bases, in one string
#define AFR_LIT_TEXT "\t" "\t*\t0\t0\t" "\tAS:i:" "\tNM:i:" "\tZS:i:" "\tMD:Z:" "\tOA:Z:" ",+," ",-," "," ";" "\tAA:Z:" "\n" "\t4\t*\t0\t255\t*\t*\t0\t0\t" "*" "^" "MIDNSHP=X" "ACGTN"
#define AFR_LIT_BYTES 89
static_assert(sizeof(AFR_LIT_TEXT) == AFR_LIT_BYTES, "literal table");
enum { LT_TAB = 0, LT_MATE = 1, LT_AS = 8, LT_NM = 14, LT_ZS = 20, LT_MD = 26, LT_OA = 32, LT_PLUS = 38, LT_MINUS = 41, LT_COMMA = 44, LT_SEMI = 45, LT_AA = 46, LT_NL = 52,
       LT_UNAL = 53, LT_STAR = 72, LT_CARET = 73, LT_OPS = 74, LT_BASES = 83 };
enum { SK_LIT = 0, SK_NUM, SK_NEG, SK_NAME, SK_RNAME, SK_SEQ, SK_QUAL, SK_CIG, SK_MD };

// the words of a recipe's header (finish_prep_kernel writes them, one lane of finish_render_kernel holds each)
enum { AFP_H_FLAGS = 0, AFP_H_NCIG, AFP_H_NMD, AFP_H_NM, AFP_H_LIFTNM, AFP_H_MAPQ, AFP_H_SCORE, AFP_H_SCORE2, AFP_H_POS1, AFP_H_OAPOS, AFP_H_SIDS, AFP_H_LIFTED_LO, AFP_H_LIFTED_HI,
       AFP_H_POS_LO, AFP_H_POS_HI, AFP_H_N };
enum { AFP_F_ALIGNED = 1u, AFP_F_MAPPED = 2u, AFP_F_STRAND = 4u, AFP_F_HOST = 8u };
#define AFP_ALT 16u              // 3 words per alternative: sequence, 1-based position, score

#define AFR_LINE_BYTES 1280u     // bytes of one line in LDS (AFS_LINE): a longer line is the host pipeline's
AFR_HD bool afr_fits(uint32_t p) { return p <= AFR_LINE_BYTES; }
#define AFR_NFIX 35u             // segments of the fixed skeleton
// an entry of the segment table: kind | header word << 4 | literal offset << 8 | literal length << 16 | AFR_T_* bits
enum { AFR_T_MAPPED0 = 1u << 20,          // a number that is 0 when the read is not mapped
       AFR_T_STAR_UNMAPPED = 1u << 21,    // "*" when the read is not mapped
       AFR_T_STAR_NOQUAL = 1u << 22,      // "*" when the batch has no qualities
       AFR_T_ZS = 1u << 23,               // empty when score2 == 0
       AFR_T_FLAG = 1u << 24,             // the SAM flag: 16 on the reverse strand, else 0
       AFR_T_HI16 = 1u << 25,             // the name id is the header word's upper half (else the lower)
       AFR_T_SIGN = 1u << 26,             // the literal ",+,": "-" on the reverse strand
       AFR_T_LIFTED = 1u << 27 };         // the lifted CIGAR (else the stitched one)
#define AFR_E_LIT(at, len) ((uint32_t)SK_LIT | ((uint32_t)(at) << 8) | ((uint32_t)(len) << 16))
#define AFR_E_NUM(word) ((uint32_t)SK_NUM | ((uint32_t)(word) << 4))
#define AFR_E_KIND(kind) ((uint32_t)(kind))
#define AFR_TAB_INIT { \
    AFR_E_KIND(SK_RNAME), AFR_E_LIT(LT_TAB, 1), AFR_E_NUM(AFP_H_FLAGS) | AFR_T_FLAG, AFR_E_LIT(LT_TAB, 1), \
    AFR_E_KIND(SK_NAME) | (AFP_H_SIDS << 4) | AFR_T_HI16 | AFR_T_STAR_UNMAPPED, AFR_E_LIT(LT_TAB, 1), AFR_E_NUM(AFP_H_POS1) | AFR_T_MAPPED0, AFR_E_LIT(LT_TAB, 1), \
    AFR_E_NUM(AFP_H_MAPQ), AFR_E_LIT(LT_TAB, 1), AFR_E_KIND(SK_CIG) | AFR_T_LIFTED | AFR_T_STAR_UNMAPPED, AFR_E_LIT(LT_MATE, 7), \
    AFR_E_KIND(SK_SEQ), AFR_E_LIT(LT_TAB, 1), AFR_E_KIND(SK_QUAL) | AFR_T_STAR_NOQUAL, AFR_E_LIT(LT_AS, 6), \
    AFR_E_NUM(AFP_H_SCORE), AFR_E_LIT(LT_NM, 6), AFR_E_NUM(AFP_H_NM) | AFR_T_MAPPED0, AFR_E_LIT(LT_ZS, 6) | AFR_T_ZS, \
    AFR_E_NUM(AFP_H_SCORE2) | AFR_T_ZS, AFR_E_LIT(LT_MD, 6), AFR_E_KIND(SK_MD), AFR_E_LIT(LT_OA, 6), \
    AFR_E_KIND(SK_NAME) | (AFP_H_SIDS << 4), AFR_E_LIT(LT_COMMA, 1), AFR_E_NUM(AFP_H_OAPOS), AFR_E_LIT(LT_PLUS, 3) | AFR_T_SIGN, \
    AFR_E_KIND(SK_CIG), AFR_E_LIT(LT_COMMA, 1), AFR_E_NUM(AFP_H_MAPQ), AFR_E_LIT(LT_COMMA, 1), \
    AFR_E_NUM(AFP_H_LIFTNM), AFR_E_LIT(LT_SEMI, 1), AFR_E_LIT(LT_AA, 6) }
// the skeleton's segments that all lanes write together: where they sit in it
enum { AFR_SEG_RNAME = 0, AFR_SEG_REF = 4, AFR_SEG_OA = 24, AFR_SEG_LCIG = 10, AFR_SEG_SEQ = 12, AFR_SEG_QUAL = 14, AFR_SEG_MD = 22, AFR_SEG_CIG = 28 };

// what is the same for every lane of a read
struct afr_read_t {
    uint32_t mapped, strand, has_q, has_zs;      // 0 / 1
    uint32_t rname_len, m, w_lcig, w_cig, w_md;  // lengths of the segments that are not one lane's
};
// a segment as its lane knows it.  SK_LIT: lit holds its bytes, lowest first (at most 7).  SK_NUM / SK_NEG: val is the magnitude.  SK_NAME: val is the
// sequence id and len is still to be looked up.
struct afr_seg_t { uint32_t kind, val, len; uint64_t lit; };

AFR_HD uint32_t afr_ndig(uint32_t u) {
    return 1u + (u >= 10u) + (u >= 100u) + (u >= 1000u) + (u >= 10000u) + (u >= 100000u) + (u >= 1000000u) + (u >= 10000000u) + (u >= 100000000u) + (u >= 1000000000u);
}
// the first len (at most 8) bytes of the literal table from `at`, lowest byte first
AFR_HD uint64_t afr_lit8(const char* lit, uint32_t at, uint32_t len) {
    uint64_t x = 0;
    for (uint32_t d = 0; d < len && d < 8; ++d) x |= (uint64_t)(uint8_t)lit[at + d] << (8 * d);
    return x;
}
AFR_HD void afr_as_num(afr_seg_t& s, int32_t v) {
    if (v < 0) { s.kind = SK_NEG; s.val = 0u - (uint32_t)v; s.len = afr_ndig(s.val) + 1u; }
    else { s.kind = SK_NUM; s.val = (uint32_t)v; s.len = afr_ndig(s.val); }
}
// segment i < AFR_NFIX of an aligned record: e is afr_tab[i], lit its literal's bytes (afr_lit8 of the entry: they never change), raw the header word the entry names
AFR_HD afr_seg_t afr_fixed_seg(uint32_t e, uint64_t lit, uint32_t raw, const afr_read_t& R) {
    afr_seg_t s;
    s.kind = e & 0xFu; s.val = 0; s.len = (e >> 16) & 0xFu; s.lit = lit;
    const bool star = ((e & AFR_T_STAR_UNMAPPED) && !R.mapped) || ((e & AFR_T_STAR_NOQUAL) && !R.has_q);
    if (s.kind == SK_NUM) {
        int32_t v = (int32_t)raw;
        if (e & AFR_T_FLAG) v = R.strand ? 16 : 0;
        if ((e & AFR_T_MAPPED0) && !R.mapped) v = 0;
        afr_as_num(s, v);
    }
    else if (s.kind == SK_NAME) s.val = (e & AFR_T_HI16) ? raw >> 16 : raw & 0xFFFFu;
    else if (s.kind == SK_RNAME) s.len = R.rname_len;
    else if (s.kind == SK_SEQ || s.kind == SK_QUAL) s.len = R.m;
    else if (s.kind == SK_CIG) s.len = (e & AFR_T_LIFTED) ? R.w_lcig : R.w_cig;
    else if (s.kind == SK_MD) s.len = R.w_md;
    else if ((e & AFR_T_SIGN) && R.strand) s.lit ^= (uint64_t)('+' ^ '-') << 8;
    if (star) { s.kind = SK_LIT; s.len = 1; s.lit = '*'; }
    if ((e & AFR_T_ZS) && !R.has_zs) { s.kind = SK_LIT; s.len = 0; }
    return s;
}
// segment i >= AFR_NFIX: "name,pos,score;" per alternative, then the newline.  Which word of the recipe a lane needs (afr_alt_word) and what it makes of it.
AFR_HD uint32_t afr_alt_word(uint32_t i) { const uint32_t j = i - AFR_NFIX, k = j / 6u, x = j - 6u * k; return AFP_ALT + 3u * k + (x >> 1); }
AFR_HD afr_seg_t afr_alt_seg(uint32_t i, uint32_t n_alt, uint32_t raw) {
    afr_seg_t s;
    const uint32_t j = i - AFR_NFIX, x = j % 6u;
    s.kind = SK_LIT; s.val = 0; s.len = 1; s.lit = x == 5u ? ';' : ',';
    if (j >= 6u * n_alt) { s.lit = '\n'; s.len = j == 6u * n_alt ? 1u : 0u; }
    else if (x == 0u) { s.kind = SK_NAME; s.val = raw; }
    else if (!(x & 1u)) afr_as_num(s, (int32_t)raw);
    return s;
}
// the bytes of a literal (at most 7) and of a number, written by the lane that owns the segment
AFR_HD void afr_put_lit(uint8_t* dst, uint64_t lit, uint32_t len) {
    AFR_UNROLLED for (uint32_t d = 0; d < 7; ++d) if (d < len) dst[d] = (uint8_t)(lit >> (8 * d));
}
AFR_HD void afr_put_digits(uint8_t* dst, uint32_t u, uint32_t nd) {          // one division per digit
    AFR_ROLLED for (uint32_t t = nd; t-- > 0;) { dst[t] = (uint8_t)('0' + u % 10u); u /= 10u; }
}
AFR_HD void afr_put_num(uint8_t* dst, uint32_t kind, uint32_t u, uint32_t len) {
    if (kind == SK_NEG) { dst[0] = '-'; afr_put_digits(dst + 1, u, len - 1u); }
    else afr_put_digits(dst, u, len);
}
// one CIGAR operation (length << 4 | operation): its length, then its letter
AFR_HD uint32_t afr_cig_len(uint32_t op) { return afr_ndig(op >> 4) + 1u; }
AFR_HD void afr_put_cig(uint8_t* dst, uint32_t op, const char* lit) {
    const uint32_t nd = afr_ndig(op >> 4);
    afr_put_digits(dst, op >> 4, nd);
    dst[nd] = (uint8_t)lit[LT_OPS + (op & 0xFu)];
}
// one MD item: type (0 closing count, 1 mismatch, 2 deletion) | matches before it << 2 | mismatch: reference base << 12; deletion: length << 12 | offset of its
// first base in the reference window << 21.  Its text: the count, then the base, or ^ and the deleted bases (base(j): the 0 .. 4 code of the j-th of them)
AFR_HD uint32_t afr_md_len(uint32_t it) {
    const uint32_t ty = it & 3u;
    return afr_ndig((it >> 2) & 0x3FFu) + (ty == 1u ? 1u : ty == 2u ? 1u + ((it >> 12) & 0x1FFu) : 0u);
}
template <class BaseF>
AFR_HD void afr_put_md(uint8_t* dst, uint32_t it, const char* lit, BaseF base) {
    const uint32_t ty = it & 3u, run = (it >> 2) & 0x3FFu, nd = afr_ndig(run);
    afr_put_digits(dst, run, nd);
    if (ty == 1u) { const uint32_t bc = (it >> 12) & 7u; dst[nd] = (uint8_t)lit[LT_BASES + (bc > 4u ? 4u : bc)]; }
    else if (ty == 2u) {
        dst[nd] = '^';
        const uint32_t dl = (it >> 12) & 0x1FFu;
        AFR_ROLLED for (uint32_t j = 0; j < dl; ++j) dst[nd + 1u + j] = (uint8_t)lit[LT_BASES + base((it >> 21) + j)];
    }
}
