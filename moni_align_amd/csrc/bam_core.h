// Per-line code of the BAM encoder: one SAM line = one BAM record, made by one wavefront of BAM_W lanes.  The file compiles
// for the host with the lanes as loops (tests/host_sim/bam_sim.cpp), as bgzf_core.h does: what depends on the lane stands in a BAM_LANES loop
// or behind BAM_ONE (one lane stores), everything else is the same for all lanes of the wave (the line's bounds come from a wave-uniform
// index, field boundaries from ballots), so the branches are scalar and the host runs that code once.  Only bam_ballot_eq differs between the
// two builds.  Every lane writes its own bytes and no byte twice, so the record is a function of the line and the dictionary alone.
//
// A line [s, e) (e: its \n) goes through bam_line twice, with the same code: bam_line<false> checks it and gives the record's size (the size
// pass; a scan of the sizes places the records), bam_line<true> writes the record at its offset.  Inside:
//   fields   ten searches for \t, 64 bytes a step (a ballot, the first set bit); QUAL ends at the next \t or at e
//   numbers  FLAG POS MAPQ PNEXT TLEN and the i tags: -?[0-9]+ folded by the wave as one, range-checked
//   names    RNAME / RNEXT: FNV-1a of the bytes into the open-addressing table of the header's @SQ names, a hit confirmed byte by byte
//   CIGAR    the bytes walked by the wave as one: digits fold, a letter closes an op (one lane stores it), M D N = X add to the reference length
//   QNAME    lane l copies bytes l, l + 64, ...;  SEQ: lane l packs bases 2j and 2j + 1 into byte j = l, l + 64, ...;  QUAL: byte j - 33
//   tags     one at a time: A one byte, i the smallest type in htslib's order, Z copied by the lanes
//   header   the 36 fixed bytes last (block_size is known by then), byte by byte: a record starts at any offset, so no word store fits
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/moni_hip.h"

#ifndef MONI_HD
#if defined(__HIPCC__)
#define MONI_HD __host__ __device__ __forceinline__
#else
#define MONI_HD inline
#endif
#endif

#define BAM_W 64u                   // lanes of a line's wavefront
#define BAM_T 256u                  // lanes of a workgroup: four lines at a time
#define BAM_TILE 1024u              // bytes of text a wavefront takes in the two newline passes
#define BAM_MAX_LINE (1u << 28)     // bytes of a line: l_seq and every size of a record stay far inside 32 bits
#define BAM_MAX_NAME 254u
#define BAM_MAX_OPS 65535u
#define BAM_MAX_OPLEN (1u << 28)
#define BAM_FIXED 36u               // block_size and the 32 bytes of fixed fields
#define BAM_NO_REF (-2)

#if defined(__HIP_DEVICE_COMPILE__)
#define BAM_LANES(l) for (uint32_t l = threadIdx.x & (BAM_W - 1u), once_ = 1; once_; once_ = 0)
#define BAM_ONE() if ((threadIdx.x & (BAM_W - 1u)) == 0)
#else
#define BAM_LANES(l) for (uint32_t l = 0; l < BAM_W; ++l)
#define BAM_ONE()
#endif
#if defined(__HIPCC__)
#define BAM_FN __host__ __device__ __forceinline__          // the host half of the library parses the header with the same pieces
#else
#define BAM_FN inline
#endif

// the dictionary of the header's @SQ lines: slot = id + 1 of a name whose hash probes to it, 0 = free; at most half the slots are taken
typedef struct { uint32_t name_off, name_len; } bam_ref_t;
typedef struct { const uint8_t* names; const bam_ref_t* refs; const uint32_t* slots; uint32_t mask, n_ref; } bam_dict_t;

MONI_HD uint32_t bam_fnv1a(const uint8_t* p, uint64_t n) {
    uint32_t h = 2166136261u;
    for (uint64_t i = 0; i < n; ++i) h = (h ^ p[i]) * 16777619u;
    return h;
}

// SAM specification 5.3 with arithmetic shifts on 64 bits, [beg, end): beg = -1 (an unmapped record) gives 4680
MONI_HD uint32_t bam_reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

// a base's four bits: `=ACMGRSVTWYHKDBN` in either case, 15 for every other byte.  The two constants hold the codes of the letters by their
// low five bits (A = 1 ... Z = 26), a nibble each.
MONI_HD uint32_t bam_base4(uint8_t c) {
    if (c == '=') return 0;
    if ((uint32_t)((c | 0x20u) - 'a') >= 26u) return 15u;
    const uint32_t i = c & 31u;
    return (uint32_t)(((i < 16u ? 0xFF3FCFFB4FFD2E1Full : 0xFFFFFFAF97F865FFull) >> (4u * (i & 15u))) & 15u);
}

// MIDNSHP=X -> 0..8, 9 for every other byte
MONI_HD uint32_t bam_cigar_op(uint8_t c) {
    switch (c) {
        case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
        case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8; default: return 9;
    }
}

// the lanes l whose byte t[at + l], below end, is ch
BAM_FN uint64_t bam_ballot_eq(const uint8_t* t, uint64_t at, uint64_t end, uint8_t ch) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint64_t q = at + (threadIdx.x & (BAM_W - 1u));
    return __ballot(q < end && t[q] == ch);
#else
    uint64_t m = 0;
    for (uint32_t l = 0; l < BAM_W; ++l)
        if (at + l < end && t[at + l] == ch) m |= 1ull << l;
    return m;
#endif
}

// the first ch in [from, end), or end
BAM_FN uint64_t bam_find(const uint8_t* t, uint64_t from, uint64_t end, uint8_t ch) {
    for (uint64_t p = from; p < end; p += BAM_W) {
        const uint64_t m = bam_ballot_eq(t, p, end, ch);
        if (m) return p + (uint64_t)__builtin_ctzll(m);
    }
    return end;
}

// ---- the two newline passes: line k + 1 starts behind the k-th \n --------------------------------------------------------------------
BAM_FN uint64_t bam_tile_count(const uint8_t* t, uint64_t len, uint64_t tile) {
    const uint64_t a = tile * BAM_TILE, b = a + BAM_TILE < len ? a + BAM_TILE : len;
    uint64_t n = 0;
    for (uint64_t p = a; p < b; p += BAM_W) n += (uint64_t)__builtin_popcountll(bam_ballot_eq(t, p, b, '\n'));
    return n;
}
// base: the \n before the tile (the exclusive scan of the counts); starts has room for one entry more than there are \n in the text
BAM_FN void bam_tile_starts(const uint8_t* t, uint64_t len, uint64_t tile, uint64_t base, uint64_t* starts) {
    const uint64_t a = tile * BAM_TILE, b = a + BAM_TILE < len ? a + BAM_TILE : len;
    for (uint64_t p = a; p < b; p += BAM_W) {
        const uint64_t m = bam_ballot_eq(t, p, b, '\n');
        BAM_LANES(l) {
            if ((m >> l) & 1u) starts[base + (uint64_t)__builtin_popcountll(m & ((1ull << l) - 1u)) + 1u] = p + l + 1u;
        }
        base += (uint64_t)__builtin_popcountll(m);
    }
}

// ---- pieces of a line --------------------------------------------------------------------------------------------------------------------
// -?[0-9]+ in [lo, hi], both within [-2^33, 2^33]: the fold saturates at 2^33, so any number of digits is taken
BAM_FN bool bam_int(const uint8_t* t, uint64_t a, uint64_t b, int64_t lo, int64_t hi, int64_t& v) {
    const bool neg = a < b && t[a] == '-';
    if (neg) ++a;
    if (a >= b) return false;
    int64_t x = 0;
    for (; a < b; ++a) {
        const uint32_t d = (uint32_t)t[a] - '0';
        if (d > 9u) return false;
        x = x * 10 + (int64_t)d;
        if (x > (1ll << 33)) x = 1ll << 33;
    }
    v = neg ? -x : x;
    return v >= lo && v <= hi;
}

// the id of the name t[a, b) in the dictionary, or BAM_NO_REF
BAM_FN int32_t bam_ref_id(const bam_dict_t& D, const uint8_t* t, uint64_t a, uint64_t b) {
    const uint64_t n = b - a;
    uint32_t h = bam_fnv1a(t + a, n) & D.mask;
    for (uint32_t probe = 0; probe <= D.mask; ++probe, h = (h + 1u) & D.mask) {
        const uint32_t v = D.slots[h];
        if (!v) return BAM_NO_REF;
        const bam_ref_t r = D.refs[v - 1u];
        if (r.name_len != n) continue;
        bool same = true;
        for (uint64_t i = 0; i < n && same; ++i) same = D.names[r.name_off + i] == t[a + i];
        if (same) return (int32_t)(v - 1u);
    }
    return BAM_NO_REF;
}

BAM_FN void bam_put16(uint8_t* o, uint32_t v) { o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); }
BAM_FN void bam_put32(uint8_t* o, uint32_t v) { o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)(v >> 16); o[3] = (uint8_t)(v >> 24); }

#define BAM_BAD(r) do { why = (r); return 0; } while (0)

// The line t[s, e) (e: its \n).  Returns the bytes of its record, block_size's four included, or 0 with `why` set for a bad line.
// WRITE: the record goes to out[0, that size); a line the size pass took is never bad here.
template <bool WRITE>
BAM_FN uint64_t bam_line(const uint8_t* t, uint64_t s, uint64_t e, const bam_dict_t& D, uint8_t* out, uint32_t& why) {
    why = MONI_BAM_OK;
    if (e - s >= BAM_MAX_LINE) BAM_BAD(MONI_BAM_LENGTH);
    if (s < e && t[s] == '@') BAM_BAD(MONI_BAM_AT);
    uint64_t f[11];          // f[k]: where field k begins; fields 0..9 end one byte before the next begins
    f[0] = s;
#pragma unroll
    for (int k = 1; k < 11; ++k) {
        const uint64_t tab = bam_find(t, f[k - 1], e, '\t');
        if (tab == e) BAM_BAD(MONI_BAM_FIELDS);
        f[k] = tab + 1u;
    }
    const uint64_t qual_end = bam_find(t, f[10], e, '\t');
    const uint32_t l_name = (uint32_t)(f[1] - 1u - f[0]);
    if (l_name == 0 || l_name > BAM_MAX_NAME) BAM_BAD(MONI_BAM_QNAME);
    int64_t flag, pos, mapq, pnext, tlen;
    if (!bam_int(t, f[1], f[2] - 1u, 0, 65535, flag) || !bam_int(t, f[3], f[4] - 1u, 0, 0x7FFFFFFFll, pos) || !bam_int(t, f[4], f[5] - 1u, 0, 255, mapq) ||
        !bam_int(t, f[7], f[8] - 1u, 0, 0x7FFFFFFFll, pnext) || !bam_int(t, f[8], f[9] - 1u, -0x7FFFFFFFll, 0x7FFFFFFFll, tlen))
        BAM_BAD(MONI_BAM_INT);
    int32_t ref = -1, next_ref = -1;
    if (!(f[3] - 1u - f[2] == 1u && t[f[2]] == '*') && (ref = bam_ref_id(D, t, f[2], f[3] - 1u)) == BAM_NO_REF) BAM_BAD(MONI_BAM_RNAME);
    if (f[7] - 1u - f[6] == 1u && t[f[6]] == '=') next_ref = ref;
    else if (!(f[7] - 1u - f[6] == 1u && t[f[6]] == '*') && (next_ref = bam_ref_id(D, t, f[6], f[7] - 1u)) == BAM_NO_REF) BAM_BAD(MONI_BAM_RNAME);

    // CIGAR, behind the name and its NUL
    const uint64_t cig = BAM_FIXED + l_name + 1u;          // offsets in the record
    uint32_t n_ops = 0;
    uint64_t reflen = 0;
    {
        const uint64_t a = f[5], b = f[6] - 1u;
        if (a == b) BAM_BAD(MONI_BAM_CIGAR);
        if (!(b - a == 1u && t[a] == '*')) {
            uint32_t x = 0, digits = 0;
            for (uint64_t p = a; p < b; ++p) {
                const uint8_t c = t[p];
                const uint32_t d = (uint32_t)c - '0';
                if (d <= 9u) {
                    x = x * 10u + d;
                    if (x > BAM_MAX_OPLEN) x = BAM_MAX_OPLEN;
                    digits = 1;
                    continue;
                }
                const uint32_t op = bam_cigar_op(c);
                if (op > 8u || !digits || x >= BAM_MAX_OPLEN || n_ops == BAM_MAX_OPS) BAM_BAD(MONI_BAM_CIGAR);
                if (WRITE) {
                    BAM_ONE() bam_put32(out + cig + 4u * (uint64_t)n_ops, x << 4 | op);
                }
                if ((0x18Du >> op) & 1u) reflen += x;          // M D N = X
                ++n_ops;
                x = 0; digits = 0;
            }
            if (digits) BAM_BAD(MONI_BAM_CIGAR);
        }
    }

    // SEQ and QUAL
    const uint64_t sa = f[9], sb = f[10] - 1u, qa = f[10];
    if (sa == sb) BAM_BAD(MONI_BAM_SEQ);
    const uint32_t l_seq = sb - sa == 1u && t[sa] == '*' ? 0u : (uint32_t)(sb - sa);
    const bool no_qual = qual_end - qa == 1u && t[qa] == '*';
    if (!no_qual && qual_end - qa != l_seq) BAM_BAD(MONI_BAM_QUAL);
    const uint64_t seq = cig + 4u * (uint64_t)n_ops, qual = seq + (l_seq + 1u) / 2u;
    if (WRITE) {
        BAM_LANES(l) {
            for (uint32_t j = l; j < l_name; j += BAM_W) out[BAM_FIXED + j] = t[s + j];
            for (uint32_t j = l; j < (l_seq + 1u) / 2u; j += BAM_W)
                out[seq + j] = (uint8_t)(bam_base4(t[sa + 2u * j]) << 4 | (2u * j + 1u < l_seq ? bam_base4(t[sa + 2u * j + 1u]) : 0u));
            for (uint32_t j = l; j < l_seq; j += BAM_W) out[qual + j] = no_qual ? (uint8_t)0xFF : (uint8_t)(t[qa + j] - 33u);
        }
        BAM_ONE() out[BAM_FIXED + l_name] = 0;
    }

    // tags: p stands on the \t before one
    uint64_t tg = qual + l_seq;
    for (uint64_t p = qual_end; p < e;) {
        const uint64_t a = p + 1u, b = bam_find(t, a, e, '\t');
        if (b - a < 5u || t[a + 2u] != ':' || t[a + 4u] != ':') BAM_BAD(MONI_BAM_TAG);
        const uint8_t ty = t[a + 3u];
        uint32_t n_val;          // bytes behind the tag's two letters and its type
        uint8_t bam_ty = ty;
        if (ty == 'A') {
            if (b - a != 6u) BAM_BAD(MONI_BAM_TAG);
            n_val = 1;
            if (WRITE) {
                BAM_ONE() out[tg + 3u] = t[a + 5u];
            }
        } else if (ty == 'i') {
            int64_t v;
            if (!bam_int(t, a + 5u, b, -(1ll << 31), (1ll << 32) - 1, v)) BAM_BAD(MONI_BAM_TAGINT);
            if (v >= 0) { bam_ty = v <= 255 ? 'C' : v <= 65535 ? 'S' : 'I'; n_val = v <= 255 ? 1u : v <= 65535 ? 2u : 4u; }
            else { bam_ty = v >= -128 ? 'c' : v >= -32768 ? 's' : 'i'; n_val = v >= -128 ? 1u : v >= -32768 ? 2u : 4u; }
            if (WRITE) {
                BAM_ONE() {
                    const uint32_t u = (uint32_t)(int32_t)v;          // two's complement: the low bytes are the narrower types'
                    if (n_val == 1u) out[tg + 3u] = (uint8_t)u;
                    else if (n_val == 2u) bam_put16(out + tg + 3u, u);
                    else bam_put32(out + tg + 3u, u);
                }
            }
        } else if (ty == 'Z') {
            const uint32_t n = (uint32_t)(b - a - 5u);
            n_val = n + 1u;
            if (WRITE) {
                BAM_LANES(l) {
                    for (uint32_t j = l; j < n; j += BAM_W) out[tg + 3u + j] = t[a + 5u + j];
                }
                BAM_ONE() out[tg + 3u + n] = 0;
            }
        } else BAM_BAD(MONI_BAM_TAGTYPE);
        if (WRITE) {
            BAM_ONE() { out[tg] = t[a]; out[tg + 1u] = t[a + 1u]; out[tg + 2u] = bam_ty; }
        }
        tg += 3u + n_val;
        p = b;
    }

    const uint64_t total = tg;
    if (WRITE) {
        BAM_ONE() {
            const int64_t beg = pos - 1;
            bam_put32(out, (uint32_t)(total - 4u));
            bam_put32(out + 4, (uint32_t)ref);
            bam_put32(out + 8, (uint32_t)(int32_t)beg);
            out[12] = (uint8_t)(l_name + 1u);
            out[13] = (uint8_t)mapq;
            bam_put16(out + 14, bam_reg2bin(beg, beg + (int64_t)(reflen ? reflen : 1u)) & 0xFFFFu);
            bam_put16(out + 16, n_ops);
            bam_put16(out + 18, (uint32_t)flag);
            bam_put32(out + 20, l_seq);
            bam_put32(out + 24, (uint32_t)next_ref);
            bam_put32(out + 28, (uint32_t)(int32_t)(pnext - 1));
            bam_put32(out + 32, (uint32_t)(int32_t)tlen);
        }
    }
    return total;
}

// ---- host side: the BAM header and the dictionary of a SAM header's @SQ lines (moni_bam_set_header, tests/host_sim/bam_sim.cpp) -------
#include <vector>

struct bam_header_t {
    std::vector<uint8_t> bam;          // magic, l_text, the text as given, n_ref, then l_name, name, NUL, l_ref per @SQ line
    std::vector<uint8_t> names;        // the names one behind the other
    std::vector<bam_ref_t> refs;
    std::vector<uint32_t> slots;       // a power of two, at least 8 and at least twice the names
};

// false: an @SQ line without SN: or with an LN: outside [1, 2^31), a name of more than BAM_MAX_NAME bytes or none, a text of 2^31 bytes or more.
// A name that comes twice keeps its first id.
inline bool bam_header_build(const char* text, uint64_t len, bam_header_t& H) {
    if (len >= (1ull << 31)) return false;
    H.bam.clear(); H.names.clear(); H.refs.clear(); H.slots.clear();
    std::vector<uint32_t> l_ref;
    const uint8_t* t = reinterpret_cast<const uint8_t*>(text);
    for (uint64_t s = 0; s < len;) {
        uint64_t e = s;
        while (e < len && t[e] != '\n') ++e;
        if (e - s >= 4 && !memcmp(t + s, "@SQ\t", 4)) {
            bool has_sn = false, has_ln = false;
            int64_t ln = 0;
            for (uint64_t a = s + 4; a <= e;) {
                uint64_t b = a;
                while (b < e && t[b] != '\t') ++b;
                if (b - a >= 3 && !memcmp(t + a, "SN:", 3) && !has_sn) {
                    if (b - a - 3 == 0 || b - a - 3 > BAM_MAX_NAME) return false;
                    H.refs.push_back(bam_ref_t{(uint32_t)H.names.size(), (uint32_t)(b - a - 3)});
                    H.names.insert(H.names.end(), t + a + 3, t + b);
                    has_sn = true;
                } else if (b - a >= 3 && !memcmp(t + a, "LN:", 3) && !has_ln) {
                    if (!bam_int(t, a + 3, b, 1, 0x7FFFFFFFll, ln)) return false;
                    has_ln = true;
                }
                a = b + 1;
            }
            if (!has_sn || !has_ln) return false;
            l_ref.push_back((uint32_t)ln);
        }
        s = e + 1;
    }
    uint32_t cap = 8;
    while (cap < 2 * H.refs.size()) cap *= 2;
    H.slots.assign(cap, 0u);
    bam_dict_t D{H.names.data(), H.refs.data(), H.slots.data(), cap - 1u, (uint32_t)H.refs.size()};
    for (uint32_t i = 0; i < H.refs.size(); ++i) {
        const bam_ref_t r = H.refs[i];
        if (bam_ref_id(D, H.names.data(), r.name_off, (uint64_t)r.name_off + r.name_len) != BAM_NO_REF) continue;
        uint32_t h = bam_fnv1a(H.names.data() + r.name_off, r.name_len) & (cap - 1u);
        while (H.slots[h]) h = (h + 1u) & (cap - 1u);
        H.slots[h] = i + 1u;
    }
    auto put32 = [&](uint32_t v) { for (int k = 0; k < 4; ++k) H.bam.push_back((uint8_t)(v >> (8 * k))); };
    H.bam.insert(H.bam.end(), {'B', 'A', 'M', 1});
    put32((uint32_t)len);
    H.bam.insert(H.bam.end(), t, t + len);
    put32((uint32_t)H.refs.size());
    for (uint32_t i = 0; i < H.refs.size(); ++i) {
        put32(H.refs[i].name_len + 1u);
        H.bam.insert(H.bam.end(), H.names.begin() + H.refs[i].name_off, H.names.begin() + H.refs[i].name_off + H.refs[i].name_len);
        H.bam.push_back(0);
        put32(l_ref[i]);
    }
    return true;
}
