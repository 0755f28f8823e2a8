// Per-member code of the BGZF reader: one BGZF member = one gzip member of at most 64 KB with any number of DEFLATE blocks
// (RFC 1951: stored, fixed, dynamic), inflated by one wavefront of INFL_T lanes into the member's own slot of the output.  The file compiles
// for the host with the lanes as loops (tests/host_sim/inflate_sim.cpp), the way bgzf_core.h does: a phase is an INFL_LANES loop, INFL_SYNC
// stands between two phases, what one phase hands the next lives in infl_shared_t (LDS on the device) or in the output slot.
//
// A member goes in rounds:
//   decode   lane 0 reads bits: block headers, code lengths, and up to INFL_RING tokens (a literal, a match, the bytes of a stored block)
//            with the output offset of each into the ring.  Every check on the bits is made here, before a token enters the ring, so
//            the lanes that execute the ring cannot leave the member's input or its output slot.  A new pair of codes ends the round.
//   execute  byte p of the round's output belongs to lane p % INFL_T.  The lane finds p's token by bisection of the ring's offsets and
//            follows matches back (byte i of a match is byte i % dist of the dist bytes before it) until it stands on a literal, on
//            a byte of a stored block (read from the input) or on a byte BEFORE the round's first (read from the output slot, where an
//            earlier round put it).  A byte of this round is never read: nothing a lane reads is written in the same phase.
//   tables   after a round that ended in a block header: the first-level lookup tables of the two codes, a lane per symbol
// then the CRC-32 of the slot by pieces (bgzf_core.h's combination), the member's status and the blocks it had by BTYPE.
#pragma once
#include "bgzf_core.h"

#define INFL_T 64u                  // lanes of a member's workgroup: one wavefront
#define INFL_RING 64u               // tokens a round decodes at most
#define INFL_MAX_OUT 65536u         // bytes a member inflates to at most (ISIZE of a BGZF member)
#define INFL_LBITS 10u              // first-level lookup: literal/length codes up to here, distance codes up to INFL_DBITS
#define INFL_DBITS 8u
#define INFL_CBITS 7u               // the code-length code, whole
#define INFL_NLIT 288u              // the fixed code has 288 literal/length and 32 distance codes; 286.. and 30.. never stand for anything
#define INFL_NDIST 32u

#define INFL_LITERAL 0u             // ring value: kind << 30 | the byte / the distance / the offset of the stored bytes in the payload
#define INFL_MATCH 1u
#define INFL_STORED 2u

#if defined(__HIP_DEVICE_COMPILE__)
#define INFL_LANES(l) for (uint32_t l = threadIdx.x, once_ = 1; once_; once_ = 0)
// between a round's stores to the output slot and the next round's loads from it: the stores have left the wave (vmcnt), the fence
// orders them for the workgroup (one CU, one L1), the barrier holds every lane of the workgroup until then
#define INFL_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __syncthreads(); } while (0)
#else
#define INFL_LANES(l) for (uint32_t l = 0; l < INFL_T; ++l)
#define INFL_SYNC() ((void)0)
#endif

// a member as the host found it (infl_member_at): where it starts in the input, where its text goes, its payload and ISIZE
struct infl_member_t {
    uint64_t in_off, out_off;
    uint32_t pay_off, pay_len;      // the DEFLATE stream: bytes [in_off + pay_off, + pay_len); CRC-32 and ISIZE follow it
    uint32_t isize, pad;
};

struct infl_args_t {
    const uint8_t* in;              // the members, back to back
    const infl_member_t* mem; uint64_t n_members;
    uint8_t* out;                   // slot of member b: min(isize, INFL_MAX_OUT) bytes at out_off
    uint32_t* status;               // per member: MONI_INF_*
    unsigned long long* counters;   // DEFLATE blocks seen: [0] stored [1] fixed [2] dynamic
    uint32_t check_crc;
};

struct infl_shared_t {
    uint16_t ltab[1u << INFL_LBITS], dtab[1u << INFL_DBITS];      // low bits of the stream -> symbol << 4 | code length; 0: a longer code, or none
    uint16_t lcnt[16], dcnt[16];                                   // codes per length
    uint16_t lsym[INFL_NLIT], dsym[INFL_NDIST];                    // symbols in the order of their codes
    uint16_t lcode[INFL_NLIT], dcode[INFL_NDIST];                  // a symbol's code, bit-reversed
    uint16_t nxt[16], offs[16];
    uint8_t llen[INFL_NLIT + INFL_NDIST], dlen[INFL_NDIST], clen[20];
    uint32_t crc_tab[256];
    uint32_t off[INFL_RING + 1], val[INFL_RING];                   // the ring: token k makes the bytes [off[k], off[k + 1]) of the slot
    uint64_t acc;                                                  // lane 0's bit reader between rounds
    uint32_t nb, at;
    uint32_t out, ntok, in_block, last, build, done, reason, crc;
    uint32_t nblk[3];
};

// ---- the members of a stream (host and device) -----------------------------------------------------------------------------------------
// The member that starts at d[at]: 0 and m filled in (out_off is the caller's), 1 when it is not whole within len, 2 when it is no BGZF
// member: ID1 ID2 CM FLG are 1f 8b 08 04, the extra field holds a `BC` subfield of 2 bytes - anywhere in it -, and BSIZE leaves room for
// the header and the trailer.
MONI_HD int infl_member_at(const uint8_t* d, uint64_t len, uint64_t at, infl_member_t& m) {
    if (len - at < 12u) return 1;
    const uint8_t* h = d + at;
    if (h[0] != 0x1Fu || h[1] != 0x8Bu || h[2] != 8u || h[3] != 4u) return 2;
    const uint32_t xlen = (uint32_t)h[10] | ((uint32_t)h[11] << 8);
    if (len - at < 12u + (uint64_t)xlen) return 1;
    uint32_t total = 0;
    for (uint32_t x = 0; x + 4u <= xlen;) {
        const uint32_t slen = (uint32_t)h[12u + x + 2u] | ((uint32_t)h[12u + x + 3u] << 8);
        if (x + 4u + slen > xlen) return 2;
        if (h[12u + x] == 0x42u && h[12u + x + 1u] == 0x43u && slen == 2u) { total = ((uint32_t)h[12u + x + 4u] | ((uint32_t)h[12u + x + 5u] << 8)) + 1u; break; }
        x += 4u + slen;
    }
    if (!total || total < 12u + xlen + 8u) return 2;
    if (len - at < total) return 1;
    m.in_off = at; m.out_off = 0;
    m.pay_off = 12u + xlen; m.pay_len = total - 12u - xlen - 8u;
    const uint8_t* t = h + total - 4u;
    m.isize = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
    m.pad = 0;
    return 0;
}
MONI_HD uint32_t infl_slot_bytes(uint32_t isize) { return isize < INFL_MAX_OUT ? isize : INFL_MAX_OUT; }

// ---- bits, LSB first; past the payload's end zeros come, and infl_over says so ---------------------------------------------------------
struct infl_bits_t {
    const uint8_t* p; uint32_t n;   // the payload
    uint64_t acc; uint32_t nb, at;  // nb bits in acc; the next byte to take is p[at]
};
BGZF_FN void infl_fill(infl_bits_t& B) {          // afterwards nb >= 33
    if (B.nb <= 32u) {
        uint32_t w = 0;
        if (B.at + 4u <= B.n) memcpy(&w, B.p + B.at, 4);
        else
            for (uint32_t k = 0; k < 4u; ++k)
                if (B.at + k < B.n) w |= (uint32_t)B.p[B.at + k] << (8u * k);
        B.acc |= (uint64_t)w << B.nb;
        B.nb += 32u; B.at += 4u;
    }
}
BGZF_FN uint32_t infl_take(infl_bits_t& B, uint32_t k) {          // k <= 32, k <= nb
    const uint32_t v = (uint32_t)(B.acc & ((1ull << k) - 1ull));
    B.acc >>= k; B.nb -= k;
    return v;
}
BGZF_FN uint32_t infl_used(const infl_bits_t& B) { return 8u * B.at - B.nb; }          // bits taken so far
BGZF_FN bool infl_over(const infl_bits_t& B) { return infl_used(B) > 8u * B.n; }      // more than there are: a sequential reader ran out

// One symbol: the first-level table, then the canonical walk (a code of length L is first[L] + its rank among the codes of that length).
// -1: no code in 15 bits, which were taken.  The caller looks at infl_over first: where the bits a code took reach past the end, the
// real bits before the end held no whole code (codes are prefix-free), so a sequential reader ran out of input there.
BGZF_FN int infl_decode(infl_bits_t& B, const uint16_t* tab, uint32_t tbits, const uint16_t* cnt, const uint16_t* sym) {
    infl_fill(B);
    const uint32_t e = tab[(uint32_t)B.acc & ((1u << tbits) - 1u)];
    if (e & 15u) { infl_take(B, e & 15u); return (int)(e >> 4); }
    uint64_t a = B.acc;
    int code = 0, first = 0, index = 0;
    for (uint32_t len = 1; len <= 15u; ++len) {
        code |= (int)(a & 1u); a >>= 1;
        const int count = cnt[len];
        if (code - count < first) { infl_take(B, len); return sym[index + (code - first)]; }
        index += count; first += count;
        first <<= 1; code <<= 1;
    }
    infl_take(B, 15u);
    return -1;
}

// Lane 0: a code from its lengths.  cnt, sym (code order), code (per symbol, bit-reversed).  False where the lengths are over-subscribed,
// or incomplete with anything but no code at all or a single code of length 1 (RFC 1951 3.2.7: one distance code; zlib takes the same).
BGZF_FN bool infl_canonical(infl_shared_t& S, const uint8_t* len, uint32_t n, uint16_t* cnt, uint16_t* sym, uint16_t* code) {
    for (uint32_t i = 0; i < 16u; ++i) cnt[i] = 0;
    for (uint32_t s = 0; s < n; ++s) cnt[len[s] & 15u] += 1;
    cnt[0] = 0;
    int left = 1;
    uint32_t maxl = 0, c = 0, o = 0;
    for (uint32_t l = 1; l <= 15u; ++l) {
        left = (left << 1) - (int)cnt[l];
        if (left < 0) return false;
        if (cnt[l]) maxl = l;
        c = (c + cnt[l - 1]) << 1;
        S.nxt[l] = (uint16_t)c; S.offs[l] = (uint16_t)o;
        o += cnt[l];
    }
    if (left > 0 && maxl > 1u) return false;
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = len[s] & 15u;
        uint32_t v = 0;
        if (l) {
            sym[S.offs[l]++] = (uint16_t)s;
            uint32_t x = S.nxt[l]++;
            for (uint32_t i = 0; i < l; ++i) { v = (v << 1) | (x & 1u); x >>= 1; }
        }
        code[s] = (uint16_t)v;
    }
    return true;
}

// Lane 0: the header of a dynamic block from HLIT on; the lengths go to S.llen and S.dlen.  Returns MONI_INF_*.
BGZF_FN uint32_t infl_dynamic_header(infl_shared_t& S, infl_bits_t& B) {
    infl_fill(B);
    const uint32_t v = infl_take(B, 14u);
    if (infl_over(B)) return MONI_INF_TRUNCATED;
    const uint32_t nlit = (v & 31u) + 257u, ndist = ((v >> 5) & 31u) + 1u, ncl = (v >> 10) + 4u;
    if (nlit > 286u || ndist > 30u) return MONI_INF_CODE_LENGTHS;
    for (uint32_t i = 0; i < BGZF_NCL; ++i) S.clen[i] = 0;
    for (uint32_t i = 0; i < ncl; ++i) { infl_fill(B); S.clen[bgzf_cl_order[i]] = (uint8_t)infl_take(B, 3u); }
    if (infl_over(B)) return MONI_INF_TRUNCATED;
    // the code-length code has to be complete; its table stands in dtab until the block's own codes are built
    uint32_t kraft = 0;
    for (uint32_t i = 0; i < BGZF_NCL; ++i)
        if (S.clen[i]) kraft += 1u << (INFL_CBITS - S.clen[i]);
    if (kraft != (1u << INFL_CBITS)) return MONI_INF_CODE_LENGTHS;
    infl_canonical(S, S.clen, BGZF_NCL, S.dcnt, S.dsym, S.dcode);
    for (uint32_t s = 0; s < BGZF_NCL; ++s) {
        const uint32_t l = S.clen[s];
        if (!l) continue;
        for (uint32_t k = 0; k < (1u << (INFL_CBITS - l)); ++k) S.dtab[S.dcode[s] | (k << l)] = (uint16_t)((s << 4) | l);
    }
    const uint32_t total = nlit + ndist;
    uint32_t i = 0;
    while (i < total) {
        infl_fill(B);
        const uint32_t e = S.dtab[(uint32_t)B.acc & ((1u << INFL_CBITS) - 1u)];
        infl_take(B, e & 15u);
        if (infl_over(B)) return MONI_INF_TRUNCATED;
        const uint32_t s = e >> 4;
        if (s < 16u) { S.llen[i++] = (uint8_t)s; continue; }
        uint32_t prev = 0, rep;
        if (s == 16u) {
            if (!i) return MONI_INF_CODE_LENGTHS;
            prev = S.llen[i - 1]; rep = 3u + infl_take(B, 2u);
        } else if (s == 17u) rep = 3u + infl_take(B, 3u);
        else rep = 11u + infl_take(B, 7u);
        if (infl_over(B)) return MONI_INF_TRUNCATED;
        if (i + rep > total) return MONI_INF_CODE_LENGTHS;
        for (; rep; --rep) S.llen[i++] = (uint8_t)prev;
    }
    for (uint32_t j = 0; j < INFL_NDIST; ++j) S.dlen[j] = j < ndist ? S.llen[nlit + j] : (uint8_t)0;
    for (uint32_t j = nlit; j < INFL_NLIT; ++j) S.llen[j] = 0;
    if (!S.llen[256]) return MONI_INF_CODE_LENGTHS;
    return MONI_INF_OK;
}

// Lane 0: one round.  pay: the payload of n bytes; cap: the bytes of the slot; isize: what the trailer says.
BGZF_FN void infl_round(infl_shared_t& S, const uint8_t* pay, uint32_t n, uint32_t cap, uint32_t isize) {
    infl_bits_t B;
    B.p = pay; B.n = n; B.acc = S.acc; B.nb = S.nb; B.at = S.at;
    uint32_t out = S.out, ntok = 0, reason = MONI_INF_OK, done = 0, build = 0;
    S.off[0] = out;
    while (ntok < INFL_RING) {
        if (!S.in_block) {
            if (S.last) {          // behind the last block: nothing but the padding of its last byte, and as many bytes as ISIZE says
                if ((infl_used(B) + 7u) / 8u != n) reason = MONI_INF_TRAILING;
                else if (out != isize) reason = MONI_INF_ISIZE;
                done = 1;
                break;
            }
            infl_fill(B);
            const uint32_t hdr = infl_take(B, 3u);
            if (infl_over(B)) { reason = MONI_INF_TRUNCATED; break; }
            const uint32_t type = hdr >> 1;
            if (type == 3u) { reason = MONI_INF_BTYPE; break; }
            S.last = hdr & 1u;
            S.nblk[type] += 1;
            if (type == 0u) {
                infl_take(B, B.nb & 7u);          // to the byte boundary: at is whole bytes, so the bits before it are nb % 8
                infl_fill(B);
                const uint32_t v = infl_take(B, 32u);
                if (infl_over(B)) { reason = MONI_INF_TRUNCATED; break; }
                const uint32_t len = v & 0xFFFFu;
                if ((len ^ 0xFFFFu) != (v >> 16)) { reason = MONI_INF_STORED_LEN; break; }
                const uint32_t src = infl_used(B) >> 3, avail = n - src, room = cap - out;
                // byte by byte a reader takes a byte, then puts it: whichever runs out first is the reason
                if (len > avail && avail <= room) { reason = MONI_INF_TRUNCATED; break; }
                if (len > room) { reason = MONI_INF_OVERRUN; break; }
                if (len) {
                    S.val[ntok] = (INFL_STORED << 30) | src;
                    out += len;
                    S.off[++ntok] = out;
                }
                B.at = src + len; B.acc = 0; B.nb = 0;
                continue;
            }
            if (type == 1u) {
                for (uint32_t s = 0; s < INFL_NLIT; ++s) S.llen[s] = (uint8_t)(s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : 8u);
                for (uint32_t s = 0; s < INFL_NDIST; ++s) S.dlen[s] = 5;
            } else if ((reason = infl_dynamic_header(S, B)) != MONI_INF_OK) break;
            if (!infl_canonical(S, S.llen, INFL_NLIT, S.lcnt, S.lsym, S.lcode) || !infl_canonical(S, S.dlen, INFL_NDIST, S.dcnt, S.dsym, S.dcode)) {
                reason = MONI_INF_CODE_LENGTHS;
                break;
            }
            S.in_block = 1;
            build = 1;          // the lookup tables take every lane: the round ends here
            break;
        }
        const int s = infl_decode(B, S.ltab, INFL_LBITS, S.lcnt, S.lsym);
        if (infl_over(B)) { reason = MONI_INF_TRUNCATED; break; }
        if (s < 0) { reason = MONI_INF_BAD_SYMBOL; break; }
        if (s < 256) {
            if (out >= cap) { reason = MONI_INF_OVERRUN; break; }
            S.val[ntok] = (INFL_LITERAL << 30) | (uint32_t)s;
            out += 1;
            S.off[++ntok] = out;
            continue;
        }
        if (s == 256) { S.in_block = 0; continue; }
        if (s >= 286) { reason = MONI_INF_BAD_SYMBOL; break; }
        const uint32_t k = (uint32_t)s - 257u;
        uint32_t len;
        if (k < 8u) len = 3u + k;
        else if (k == 28u) len = 258u;
        else {
            const uint32_t eb = (k >> 2) - 1u;
            len = 3u + ((4u + (k & 3u)) << eb) + infl_take(B, eb);
            if (infl_over(B)) { reason = MONI_INF_TRUNCATED; break; }
        }
        const int d = infl_decode(B, S.dtab, INFL_DBITS, S.dcnt, S.dsym);
        if (infl_over(B)) { reason = MONI_INF_TRUNCATED; break; }
        if (d < 0 || d >= 30) { reason = MONI_INF_BAD_SYMBOL; break; }
        uint32_t dist;
        if (d < 4) dist = (uint32_t)d + 1u;
        else {
            const uint32_t eb = ((uint32_t)d >> 1) - 1u;
            dist = 1u + ((2u + ((uint32_t)d & 1u)) << eb) + infl_take(B, eb);
            if (infl_over(B)) { reason = MONI_INF_TRUNCATED; break; }
        }
        if (dist > out) { reason = MONI_INF_DISTANCE; break; }
        if (len > cap - out) { reason = MONI_INF_OVERRUN; break; }
        S.val[ntok] = (INFL_MATCH << 30) | dist;
        out += len;
        S.off[++ntok] = out;
    }
    if (reason != MONI_INF_OK) done = 1;
    S.acc = B.acc; S.nb = B.nb; S.at = B.at;
    S.out = out; S.ntok = ntok; S.build = build; S.done = done; S.reason = reason;
}

// Byte p of the round (off[0] <= p < off[ntok]), with nothing of this round read from the slot.
BGZF_FN uint8_t infl_byte(const infl_shared_t& S, const uint8_t* pay, const uint8_t* slot, uint32_t p) {
    const uint32_t start = S.off[0];
    uint32_t hi = S.ntok;
    while (p >= start) {
        uint32_t lo = 0;          // the token t < hi with off[t] <= p < off[t + 1]
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (S.off[mid] <= p) lo = mid; else hi = mid;
        }
        const uint32_t v = S.val[lo], kind = v >> 30, at = S.off[lo];
        if (kind == INFL_LITERAL) return (uint8_t)v;
        if (kind == INFL_STORED) return pay[(v & 0x3FFFFFFFu) + (p - at)];
        const uint32_t dist = v & 0x3FFFFFFFu;
        uint32_t i = p - at;
        if (i >= dist) i %= dist;
        p = at - dist + i;          // before this token: the next search is among the tokens before it
        hi = lo;
        if (!hi) break;
    }
    return slot[p];
}

// Member b, by the INFL_T lanes of one workgroup.
BGZF_FN void infl_member(infl_shared_t& S, const infl_args_t& G, uint64_t b) {
    const infl_member_t M = G.mem[b];
    const uint8_t* pay = G.in + M.in_off + M.pay_off;
    uint8_t* slot = G.out + M.out_off;
    const uint32_t n = M.pay_len, cap = infl_slot_bytes(M.isize);

    INFL_LANES(l) {
        for (uint32_t i = l; i < 256u; i += INFL_T) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ BGZF_CRC_POLY : c >> 1;
            S.crc_tab[i] = c;
        }
        if (l == 0) {
            S.acc = 0; S.nb = 0; S.at = 0;
            S.out = 0; S.ntok = 0; S.in_block = 0; S.last = 0; S.build = 0; S.done = 0; S.reason = MONI_INF_OK; S.crc = 0;
            S.nblk[0] = S.nblk[1] = S.nblk[2] = 0;
        }
    }
    INFL_SYNC();

    for (;;) {
        INFL_LANES(l) {
            if (l == 0) infl_round(S, pay, n, cap, M.isize);
        }
        INFL_SYNC();
        const uint32_t build = S.build, done = S.done;
        INFL_LANES(l) {
            const uint32_t end = S.off[S.ntok];
            for (uint32_t p = S.off[0] + l; p < end; p += INFL_T) slot[p] = infl_byte(S, pay, slot, p);
            if (build) {
                for (uint32_t i = l; i < (1u << INFL_LBITS); i += INFL_T) S.ltab[i] = 0;
                for (uint32_t i = l; i < (1u << INFL_DBITS); i += INFL_T) S.dtab[i] = 0;
            }
        }
        INFL_SYNC();
        if (build) {
            INFL_LANES(l) {
                for (uint32_t s = l; s < INFL_NLIT + INFL_NDIST; s += INFL_T) {
                    const bool lit = s < INFL_NLIT;
                    const uint32_t q = lit ? s : s - INFL_NLIT, len = lit ? S.llen[q] : S.dlen[q], bits = lit ? INFL_LBITS : INFL_DBITS;
                    if (!len || len > bits) continue;
                    uint16_t* tab = lit ? S.ltab : S.dtab;
                    const uint32_t code = lit ? S.lcode[q] : S.dcode[q];
                    for (uint32_t k = 0; k < (1u << (bits - len)); ++k) tab[code | (k << len)] = (uint16_t)((q << 4) | len);
                }
            }
            INFL_SYNC();
        }
        if (done) break;
    }

    if (G.check_crc && S.reason == MONI_INF_OK) {
        const uint32_t total = S.out;
        INFL_LANES(l) {
            const uint32_t piece = (total + INFL_T - 1u) / INFL_T;
            const uint32_t lo = l * piece < total ? l * piece : total, hi = lo + piece < total ? lo + piece : total;
            if (hi > lo) {
                uint32_t c = 0xFFFFFFFFu;
                for (uint32_t i = lo; i < hi; ++i) c = S.crc_tab[(c ^ slot[i]) & 0xFFu] ^ (c >> 8);
                bgzf_axor(&S.crc, bgzf_crc_shift(~c, total - hi));
            }
        }
        INFL_SYNC();
    }
    INFL_LANES(l) {
        if (l == 0) {
            uint32_t reason = S.reason;
            if (G.check_crc && reason == MONI_INF_OK) {
                const uint8_t* t = pay + n;
                const uint32_t want = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
                if (want != S.crc) reason = MONI_INF_CRC;
            }
            G.status[b] = reason;
            for (uint32_t k = 0; k < 3u; ++k)
                if (S.nblk[k]) bgzf_aadd64(&G.counters[k], S.nblk[k]);
        }
    }
    INFL_SYNC();
}
