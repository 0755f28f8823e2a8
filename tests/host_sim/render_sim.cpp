// render_sim.cpp: the per-lane pieces of finish_render_kernel (moni_align_amd/csrc/render_core.h: the segment table, the digits of a number, the bytes
// of a CIGAR operation and of an MD item) put together lane by lane on the host, the way the kernel puts them together, over synthetic recipes, and every
// line compared with a plain snprintf rendering of the same record.  A program of its own: tests/test_host_render.py builds it with
// -fsanitize=address,undefined and runs it.  The line buffer has exactly AFR_LINE_BYTES bytes on the heap, so a byte written past a segment's end or
// past the line is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../moni_align_amd/csrc/render_core.h"

static const char LIT[] = AFR_LIT_TEXT;
static const uint32_t TAB[AFR_NFIX] = AFR_TAB_INIT;

struct rec_t {
    bool mapped = true, strand = false, has_q = true;
    int32_t nm = 0, lift_nm = 0, mapq = 60, score = 0, score2 = 0, pos1 = 1, oa_pos = 1;
    uint32_t sid = 0, lsid = 0;
    std::vector<uint32_t> cig, lcig, md;                 // as the recipe holds them
    std::vector<uint32_t> alt_sid; std::vector<int32_t> alt_pos, alt_score;
    std::string rname, seq, qual;
};
struct world_t { std::vector<std::string> names; std::string text; uint64_t lifted = 0; };

static uint32_t nt4(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }

// ---- the reference: the record spelled with snprintf ----
static std::string num(long long v) { char b[32]; snprintf(b, sizeof b, "%lld", v); return b; }
static std::string cigar_text(const std::vector<uint32_t>& c) {
    std::string s;
    for (uint32_t op : c) { s += num(op >> 4); s += "MIDNSHP=X"[op & 0xFu]; }
    return s;
}
static std::string md_text(const std::vector<uint32_t>& md, const world_t& W) {
    std::string s;
    for (uint32_t it : md) {
        const uint32_t ty = it & 3u;
        s += num((it >> 2) & 0x3FFu);
        if (ty == 1) { const uint32_t bc = (it >> 12) & 7u; s += "ACGTN"[bc > 4 ? 4 : bc]; }
        else if (ty == 2) {
            s += '^';
            for (uint32_t j = 0; j < ((it >> 12) & 0x1FFu); ++j) { const uint64_t ta = W.lifted + (it >> 21) + j; s += "ACGTN"[nt4(ta < W.text.size() ? W.text[ta] : 'A')]; }
        }
    }
    return s;
}
static std::string want_line(const rec_t& r, const world_t& W) {
    std::string s = r.rname + "\t" + num(r.strand ? 16 : 0) + "\t" + (r.mapped ? W.names[r.lsid] : std::string("*")) + "\t" + num(r.mapped ? r.pos1 : 0) + "\t" + num(r.mapq) + "\t";
    s += (r.mapped ? cigar_text(r.lcig) : std::string("*")) + "\t*\t0\t0\t" + r.seq + "\t" + (r.has_q ? r.qual : std::string("*"));
    s += "\tAS:i:" + num(r.score) + "\tNM:i:" + num(r.mapped ? r.nm : 0);
    if (r.score2 != 0) s += "\tZS:i:" + num(r.score2);
    s += "\tMD:Z:" + md_text(r.md, W) + "\tOA:Z:" + W.names[r.sid] + "," + num(r.oa_pos) + (r.strand ? ",-," : ",+,") + cigar_text(r.cig) + "," + num(r.mapq) + "," + num(r.lift_nm) + ";";
    s += "\tAA:Z:";
    for (size_t k = 0; k < r.alt_sid.size(); ++k) s += W.names[r.alt_sid[k]] + "," + num(r.alt_pos[k]) + "," + num(r.alt_score[k]) + ";";
    return s + "\n";
}

// ---- the recipe's first 64 words as finish_prep_kernel leaves them: one per lane ----
static void header(const rec_t& r, uint32_t* hw) {
    memset(hw, 0, 64 * sizeof(uint32_t));
    hw[AFP_H_FLAGS] = AFP_F_ALIGNED | (r.mapped ? AFP_F_MAPPED : 0u) | (r.strand ? AFP_F_STRAND : 0u) | ((uint32_t)r.alt_sid.size() << 8);
    hw[AFP_H_NCIG] = (uint32_t)r.cig.size() | ((uint32_t)r.lcig.size() << 16); hw[AFP_H_NMD] = (uint32_t)r.md.size();
    hw[AFP_H_NM] = (uint32_t)r.nm; hw[AFP_H_LIFTNM] = (uint32_t)r.lift_nm; hw[AFP_H_MAPQ] = (uint32_t)r.mapq; hw[AFP_H_SCORE] = (uint32_t)r.score; hw[AFP_H_SCORE2] = (uint32_t)r.score2;
    hw[AFP_H_POS1] = (uint32_t)r.pos1; hw[AFP_H_OAPOS] = (uint32_t)r.oa_pos; hw[AFP_H_SIDS] = r.sid | (r.lsid << 16);
    for (size_t k = 0; k < r.alt_sid.size(); ++k) { hw[AFP_ALT + 3 * k] = r.alt_sid[k]; hw[AFP_ALT + 3 * k + 1] = (uint32_t)r.alt_pos[k]; hw[AFP_ALT + 3 * k + 2] = (uint32_t)r.alt_score[k]; }
}

// ---- the kernel's steps, the lanes one after the other.  false: the line does not fit (the kernel hands the read to the host) ----
static bool render(const rec_t& r, const world_t& W, std::string& out) {
    uint32_t hw[64];
    header(r, hw);
    const uint32_t flags = hw[AFP_H_FLAGS], n_alt = (flags >> 8) & 0xFFu, n_seg = 36u + 6u * n_alt;
    afr_read_t R;
    R.mapped = (flags & AFP_F_MAPPED) ? 1u : 0u; R.strand = (flags & AFP_F_STRAND) ? 1u : 0u; R.has_q = r.has_q; R.has_zs = (int32_t)hw[AFP_H_SCORE2] != 0;
    R.rname_len = (uint32_t)r.rname.size(); R.m = (uint32_t)r.seq.size(); R.w_cig = R.w_lcig = R.w_md = 0;
    std::vector<uint32_t> c_at, l_at, d_at;          // what the scans give: where an operation's or an item's text starts in its string
    for (uint32_t op : r.cig) { c_at.push_back(R.w_cig); R.w_cig += afr_cig_len(op); }
    for (uint32_t op : r.lcig) { l_at.push_back(R.w_lcig); R.w_lcig += afr_cig_len(op); }
    for (uint32_t it : r.md) { d_at.push_back(R.w_md); R.w_md += afr_md_len(it); }
    std::vector<afr_seg_t> seg(n_seg);
    std::vector<uint32_t> at(n_seg + 1);
    uint32_t p = 0;
    for (uint32_t i = 0; i < n_seg; ++i) {          // "lane" i & 63 of pass i / 64
        afr_seg_t s;
        if (i < AFR_NFIX) { const uint32_t e = TAB[i]; s = afr_fixed_seg(e, afr_lit8(LIT, (e >> 8) & 0xFFu, (e >> 16) & 0xFu), hw[(e >> 4) & 0xFu], R); }
        else s = afr_alt_seg(i, n_alt, hw[afr_alt_word(i) & 63u]);
        if (s.kind == SK_NAME) s.len = (uint32_t)W.names[s.val].size();
        seg[i] = s; at[i] = p; p += s.len;
    }
    for (uint32_t i = n_seg; i < ((n_seg + 63u) & ~63u); ++i)          // the lanes past the last segment add nothing
        if (afr_alt_seg(i, n_alt, hw[afr_alt_word(i) & 63u]).len != 0) { fprintf(stderr, "segment %u past the newline is not empty\n", i); exit(2); }
    if (!afr_fits(p)) return false;
    uint8_t* line = (uint8_t*)malloc(AFR_LINE_BYTES);
    memset(line, '#', AFR_LINE_BYTES);
    for (uint32_t i = 0; i < n_seg; ++i) {
        const afr_seg_t& s = seg[i];
        if (s.kind == SK_LIT) afr_put_lit(line + at[i], s.lit, s.len);
        else if (s.kind == SK_NUM || s.kind == SK_NEG) afr_put_num(line + at[i], s.kind, s.val, s.len);
        else if (s.kind == SK_NAME) memcpy(line + at[i], W.names[s.val].data(), s.len);
    }
    for (size_t k = 0; k < r.cig.size(); ++k) afr_put_cig(line + at[AFR_SEG_CIG] + c_at[k], r.cig[k], LIT);
    if (R.mapped) for (size_t k = 0; k < r.lcig.size(); ++k) afr_put_cig(line + at[AFR_SEG_LCIG] + l_at[k], r.lcig[k], LIT);
    auto base_at = [&](uint32_t o) { const uint64_t ta = W.lifted + o; return nt4(ta < W.text.size() ? W.text[ta] : 'A'); };
    for (size_t k = 0; k < r.md.size(); ++k) afr_put_md(line + at[AFR_SEG_MD] + d_at[k], r.md[k], LIT, base_at);
    memcpy(line + at[AFR_SEG_SEQ], r.seq.data(), R.m);
    if (r.has_q) memcpy(line + at[AFR_SEG_QUAL], r.qual.data(), R.m);
    memcpy(line + at[AFR_SEG_RNAME], r.rname.data(), R.rname_len);
    out.assign((const char*)line, p);
    free(line);
    return true;
}

static uint64_t rng_s = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) { rng_s ^= rng_s << 13; rng_s ^= rng_s >> 7; rng_s ^= rng_s << 17; return (uint32_t)((rng_s >> 11) % n); }
static std::string letters(uint32_t n, const char* abc) { std::string s; const uint32_t k = (uint32_t)strlen(abc); for (uint32_t i = 0; i < n; ++i) s += abc[rnd(k)]; return s; }
static uint32_t md_mis(uint32_t run, uint32_t base) { return 1u | (run << 2) | (base << 12); }
static uint32_t md_del(uint32_t run, uint32_t len, uint32_t off) { return 2u | (run << 2) | (len << 12) | (off << 21); }
static uint32_t md_end(uint32_t run) { return run << 2; }

static int n_checked = 0, n_over = 0;
// renders r; expects the line of snprintf, or a hand-over exactly when that line is longer than the staging
static void check(const char* what, const rec_t& r, const world_t& W) {
    const std::string want = want_line(r, W);
    std::string got;
    const bool fits = render(r, W, got);
    ++n_checked;
    if (!fits) ++n_over;
    if (fits != (want.size() <= AFR_LINE_BYTES) || (fits && got != want)) {
        fprintf(stderr, "%s: %s\n got (%zu): %s\nwant (%zu): %s\n", what, fits ? "lines differ" : "handed over", got.size(), got.c_str(), want.size(), want.c_str());
        exit(1);
    }
}

static rec_t plain(const world_t& W, uint32_t m) {
    rec_t r;
    r.rname = "read" + num(rnd(1000000)); r.seq = letters(m, "ACGTN"); r.qual = letters(m, "!#5?IJ~");
    r.sid = rnd((uint32_t)W.names.size()); r.lsid = rnd((uint32_t)W.names.size());
    r.cig = { (m << 4) | 0u }; r.lcig = { (m << 4) | 7u }; r.md = { md_end(m) };
    r.score = (int32_t)(2 * m); r.pos1 = 1 + (int32_t)rnd(5000000); r.oa_pos = 1 + (int32_t)rnd(5000000);
    return r;
}
static void with_alts(rec_t& r, const world_t& W, uint32_t n) {
    for (uint32_t k = 0; k < n; ++k) { r.alt_sid.push_back(rnd((uint32_t)W.names.size())); r.alt_pos.push_back(1 + (int32_t)rnd(1u << (1 + rnd(30)))); r.alt_score.push_back((int32_t)rnd(600) - 100); }
}

int main() {
    world_t W;
    for (int k = 0; k < 140; ++k) W.names.push_back(k % 7 == 0 ? letters(1 + rnd(40), "abcXYZ_.0129") : "s" + num(k));
    W.text = letters(4000, "ACGTN"); W.lifted = 1000;
    // the numbers: negative AS and ZS, a 10-digit position, zeros, every digit count
    {
        rec_t r = plain(W, 150);
        r.score = -37; r.score2 = -2147483647 - 1; r.pos1 = 2147483647; r.oa_pos = 1000000000; r.nm = 0; r.lift_nm = 12; r.mapq = 0;
        check("negative AS and ZS, 10-digit positions", r, W);
        r.score2 = 0; check("score2 == 0: no ZS", r, W);
        r.score2 = 7; r.strand = true; check("reverse strand", r, W);
        r.mapped = false; r.nm = 5; r.pos1 = 77; check("not mapped: * for RNAME and CIGAR, 0 for POS and NM", r, W);
        r.has_q = false; check("no qualities", r, W);
        const int32_t pw[10] = { 1, 10, 100, 1000, 10000, 100000, 1000000, 10000000, 100000000, 1000000000 };
        for (int32_t v : pw) { r.score = v - 1; r.score2 = -v; r.lift_nm = v; r.mapq = v + 8; check("digit counts", r, W); }
    }
    // alternatives: 0, 1, 5 (the 66 segments no longer fit one pass of the lanes) and 16
    for (uint32_t n : { 0u, 1u, 4u, 5u, 15u, 16u }) { rec_t r = plain(W, 100); with_alts(r, W, n); check("alternatives", r, W); }
    // CIGARs of 64 and 128 operations, 63 / 65 / 127 too
    for (uint32_t nc : { 1u, 63u, 64u }) for (uint32_t nl : { 1u, 64u, 65u, 127u, 128u }) {
        rec_t r = plain(W, 300);
        r.cig.clear(); r.lcig.clear();
        for (uint32_t k = 0; k < nc; ++k) r.cig.push_back(((1u + rnd(k % 5 == 0 ? 500u : 12u)) << 4) | rnd(9));
        for (uint32_t k = 0; k < nl; ++k) r.lcig.push_back(((1u + rnd(k % 7 == 0 ? 1000u : 9u)) << 4) | rnd(9));
        check("long CIGARs", r, W);
    }
    // MD strings up to 256 items, deletion items among them (one of 0 bases' offset at the text's end: bases past it read as A)
    for (uint32_t nm : { 2u, 64u, 65u, 128u, 255u, 256u }) {
        rec_t r = plain(W, 60);
        r.md.clear();
        for (uint32_t k = 0; k + 1 < nm; ++k) r.md.push_back(k % 9 == 4 ? md_del(rnd(3), 1 + rnd(k % 18 == 4 ? 20u : 3u), rnd(900)) : md_mis(rnd(k % 5 ? 3u : 1000u), rnd(8)));
        r.md.push_back(md_end(rnd(1000)));
        check("long MD", r, W);
    }
    { rec_t r = plain(W, 60); r.md = { md_del(0, 6, 2997), md_end(1) }; check("deletion across the text's end", r, W); }
    // a line of exactly AFR_LINE_BYTES bytes, one byte more, and all lengths around it
    {
        rec_t r = plain(W, 512); with_alts(r, W, 3); r.rname = "";
        const size_t base = want_line(r, W).size();
        for (size_t total = AFR_LINE_BYTES - 3; total <= AFR_LINE_BYTES + 3; ++total) { r.rname = letters((uint32_t)(total - base), "qrs"); check("line capacity", r, W); }
        if (n_over != 3) { fprintf(stderr, "%d of the 7 lines around the capacity were handed over, not 3\n", n_over); return 1; }
    }
    // random records
    for (int t = 0; t < 3000; ++t) {
        rec_t r = plain(W, 1 + rnd(t % 50 == 0 ? 512u : 200u));
        r.mapped = rnd(8) != 0; r.strand = rnd(2); r.has_q = rnd(6) != 0; r.score2 = rnd(3) ? (int32_t)rnd(400) - 50 : 0; r.nm = (int32_t)rnd(40); r.lift_nm = (int32_t)rnd(40); r.mapq = (int32_t)rnd(61);
        with_alts(r, W, rnd(4) ? rnd(3) : rnd(17));
        r.cig.clear(); r.lcig.clear(); r.md.clear();
        for (uint32_t k = 0, n = 1 + rnd(rnd(6) ? 6u : 64u); k < n; ++k) r.cig.push_back(((1u + rnd(150)) << 4) | rnd(9));
        for (uint32_t k = 0, n = 1 + rnd(rnd(6) ? 8u : 128u); k < n; ++k) r.lcig.push_back(((1u + rnd(150)) << 4) | rnd(9));
        for (uint32_t k = 0, n = rnd(rnd(6) ? 8u : 255u); k < n; ++k) r.md.push_back(rnd(7) ? md_mis(rnd(120), rnd(5)) : md_del(rnd(120), 1 + rnd(8), rnd(2000)));
        r.md.push_back(md_end(rnd(200)));
        check("random record", r, W);
    }
    printf("render_sim: %d lines equal, %d of them handed over for their length\n", n_checked, n_over);
    return 0;
}
