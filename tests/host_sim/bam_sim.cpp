// bam_core.h (what the BAM encoder's kernels run per tile and per line) replayed on the host: the lanes of a wavefront as loops, the passes in
// launch order - newline counts per tile, their scan, the lines' starts, the size pass, the scan of the sizes, the write pass.  The lines go
// through the size pass LAST TO FIRST, so a later bad line is met before an earlier one: the first index is a minimum, as on the device.
// The text, the starts and the records are sized exactly, so a sanitizer build sees any byte read or written past them.
// As a library (tests/test_host_bam.py) and, with BAM_SIM_MAIN, as a stand-alone program for a sanitizer build:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DBAM_SIM_MAIN -o bam_sim_asan bam_sim.cpp && ./bam_sim_asan FILE.sam...
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../moni_align_amd/csrc/bam_core.h"

extern "C" {

// The uncompressed BAM header of a SAM header; out: room for cap bytes (MONI_ERANGE when that is too little, *out_len says how many).
int bamsim_header(const char* header, uint64_t hlen, uint8_t* out, uint64_t cap, uint64_t* out_len) {
    bam_header_t H;
    if (!out_len || (!header && hlen) || !bam_header_build(header ? header : "", hlen, H)) return MONI_EINVAL;
    *out_len = H.bam.size();
    if (H.bam.size() > cap) return MONI_ERANGE;
    memcpy(out, H.bam.data(), H.bam.size());
    return MONI_OK;
}

// The records of `text` against the dictionary of `header`.  stats: lines, BAM bytes, bad lines, the first bad line, its reason.
// Returns MONI_OK, MONI_EINVAL (a bad header, a bad line: nothing is written) or MONI_ERANGE (out is too small; stats[1] says how many).
int bamsim_records(const char* header, uint64_t hlen, const uint8_t* text, uint64_t len, uint8_t* out, uint64_t cap, uint64_t* out_len, uint64_t* stats) {
    bam_header_t H;
    if (!out_len || !stats || (!text && len) || (!header && hlen) || !bam_header_build(header ? header : "", hlen, H)) return MONI_EINVAL;
    const bam_dict_t D{H.names.data(), H.refs.data(), H.slots.data(), (uint32_t)H.slots.size() - 1u, (uint32_t)H.refs.size()};
    for (int k = 0; k < 5; ++k) stats[k] = 0;
    *out_len = 0;
    if (!len) return MONI_OK;
    if (text[len - 1] != '\n') {
        for (uint64_t i = 0; i < len; ++i) stats[3] += text[i] == '\n';
        stats[2] = 1; stats[4] = MONI_BAM_NEWLINE;
        return MONI_EINVAL;
    }
    std::unique_ptr<uint8_t[]> t(new uint8_t[len]);          // exactly len bytes: a read past the end is a read past the allocation
    memcpy(t.get(), text, len);
    const uint64_t n_tiles = (len + BAM_TILE - 1) / BAM_TILE;
    std::vector<uint64_t> cnt(n_tiles), pos(n_tiles + 1, 0);
    for (uint64_t k = 0; k < n_tiles; ++k) cnt[k] = bam_tile_count(t.get(), len, k);
    for (uint64_t k = 0; k < n_tiles; ++k) pos[k + 1] = pos[k] + cnt[k];
    const uint64_t n = pos[n_tiles];
    std::vector<uint64_t> starts(n + 1, ~0ull), size(n), off(n + 1, 0);
    starts[0] = 0;
    for (uint64_t k = n_tiles; k-- > 0;) bam_tile_starts(t.get(), len, k, pos[k], starts.data());
    uint64_t bad = 0, first = ~0ull;
    for (uint64_t i = n; i-- > 0;) {
        uint32_t why;
        size[i] = bam_line<false>(t.get(), starts[i], starts[i + 1] - 1u, D, nullptr, why);
        if (why) { ++bad; if ((i << 8 | why) < first) first = i << 8 | why; }
    }
    stats[0] = n;
    if (bad) { stats[2] = bad; stats[3] = first >> 8; stats[4] = first & 0xFFu; return MONI_EINVAL; }
    for (uint64_t i = 0; i < n; ++i) off[i + 1] = off[i] + size[i];
    stats[1] = off[n];
    *out_len = off[n];
    if (off[n] > cap) return MONI_ERANGE;
    std::unique_ptr<uint8_t[]> rec(new uint8_t[off[n] ? off[n] : 1]);
    memset(rec.get(), 0xAA, off[n]);
    for (uint64_t i = n; i-- > 0;) {
        uint32_t why;
        if (bam_line<true>(t.get(), starts[i], starts[i + 1] - 1u, D, rec.get() + off[i], why) != size[i]) return MONI_ERANGE;
    }
    memcpy(out, rec.get(), off[n]);
    return MONI_OK;
}

uint32_t bamsim_reg2bin(int64_t beg, int64_t end) { return bam_reg2bin(beg, end); }
uint32_t bamsim_base4(uint32_t c) { return bam_base4((uint8_t)c); }

}  // extern "C"

#ifdef BAM_SIM_MAIN
// the records of one text: MONI_OK (and records whose block_size fields add up to the stream) or the expected reason
static int run_case(const char* what, const std::string& header, const std::string& text, uint32_t want_reason) {
    uint64_t n = 0, st[5];
    int rc = bamsim_records(header.data(), header.size(), reinterpret_cast<const uint8_t*>(text.data()), text.size(), nullptr, 0, &n, st);
    bool ok;
    if (want_reason) ok = rc == MONI_EINVAL && st[4] == want_reason;
    else {
        std::vector<uint8_t> out(n ? n : 1);          // exactly the size
        rc = bamsim_records(header.data(), header.size(), reinterpret_cast<const uint8_t*>(text.data()), text.size(), out.data(), n, &n, st);
        ok = rc == MONI_OK;
        uint64_t at = 0, recs = 0;
        while (ok && at < n) {
            uint32_t bs;
            if (n - at < 4) { ok = false; break; }
            memcpy(&bs, out.data() + at, 4);
            at += 4 + (uint64_t)bs; ++recs;
        }
        ok = ok && at == n && recs == st[0];
    }
    printf("%-40s %9zu bytes -> rc %d, %llu lines, %llu BAM bytes, %llu bad (first %llu, reason %llu)  %s\n", what, text.size(), rc, (unsigned long long)st[0],
           (unsigned long long)st[1], (unsigned long long)st[2], (unsigned long long)st[3], (unsigned long long)st[4], ok ? "ok" : "FAILED");
    return ok ? 0 : 1;
}

int main(int argc, char** argv) {
    int bad = 0;
    const std::string hdr = "@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chr10\tLN:2000\n@SQ\tSN:chr19\tLN:600000000\n";
    auto line = [](const std::string& name, const std::string& rname, const std::string& cigar, const std::string& seq, const std::string& qual, const std::string& tags) {
        return name + "\t0\t" + rname + "\t100\t60\t" + cigar + "\t=\t200\t0\t" + seq + "\t" + qual + tags + "\n";
    };
    std::string many;
    for (int i = 0; i < 70; ++i) many += "1M1I";
    for (size_t l : {(size_t)1, (size_t)2, (size_t)63, (size_t)64, (size_t)65, (size_t)127, (size_t)129, (size_t)1000}) {
        const std::string s(l, 'A'), q(l, 'I');
        bad += run_case("l_seq", hdr, line("r", "chr19", std::to_string(l) + "M", s, q, "\tNM:i:0\tMD:Z:" + std::string(200, '7') + "\tAA:Z:"), 0);
        bad += run_case("l_seq, no QUAL", hdr, line("r", "*", "*", s, "*", ""), 0);
    }
    bad += run_case("empty", hdr, "", 0);
    bad += run_case("SEQ *", hdr, line("r", "chr1", "*", "*", "*", "\tXA:A:x"), 0);
    bad += run_case("70 ops", hdr, line(std::string(254, 'n'), "chr10", many, "ACGT", "IIII", "\tXI:i:-2147483648\tXJ:i:4294967295\tXK:i:-129\tXL:i:65536"), 0);
    bad += run_case("name of 255", hdr, line(std::string(255, 'n'), "chr10", "4M", "ACGT", "IIII", ""), MONI_BAM_QNAME);
    bad += run_case("op of 2^28", hdr, line("r", "chr1", "268435456M", "ACGT", "IIII", ""), MONI_BAM_CIGAR);
    bad += run_case("op of 2^28 - 1", hdr, line("r", "chr1", "268435455M", "ACGT", "IIII", ""), 0);
    bad += run_case("unknown RNAME", hdr, line("r", "chr2", "4M", "ACGT", "IIII", ""), MONI_BAM_RNAME);
    bad += run_case("QUAL short", hdr, line("r", "chr1", "4M", "ACGT", "III", ""), MONI_BAM_QUAL);
    bad += run_case("tag integer", hdr, line("r", "chr1", "4M", "ACGT", "IIII", "\tXI:i:4294967296"), MONI_BAM_TAGINT);
    bad += run_case("tag type", hdr, line("r", "chr1", "4M", "ACGT", "IIII", "\tXF:f:1.5"), MONI_BAM_TAGTYPE);
    bad += run_case("10 fields", hdr, "r\t0\tchr1\t1\t0\t*\t*\t0\t0\tACGT\n", MONI_BAM_FIELDS);
    bad += run_case("@ line", hdr, "@CO\tx\n", MONI_BAM_AT);
    bad += run_case("no final newline", hdr, "r\t0\tchr1\t1\t0\t*\t*\t0\t0\tACGT\tIIII", MONI_BAM_NEWLINE);
    for (int i = 1; i < argc; ++i) {
        FILE* f = fopen(argv[i], "rb");
        if (!f) { fprintf(stderr, "cannot read %s\n", argv[i]); return 2; }
        std::string all, header, text;
        char buf[65536];
        size_t k;
        while ((k = fread(buf, 1, sizeof buf, f)) > 0) all.append(buf, k);
        fclose(f);
        for (size_t s = 0; s < all.size();) {
            size_t e = all.find('\n', s);
            e = e == std::string::npos ? all.size() : e + 1;
            (all[s] == '@' ? header : text).append(all, s, e - s);
            s = e;
        }
        if (header.empty()) header = "@SQ\tSN:chr19\tLN:59128983\n";
        bad += run_case(argv[i], header, text, 0);
    }
    printf("%d case(s) failed\n", bad);
    return bad ? 1 : 0;
}
#endif
