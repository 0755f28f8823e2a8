// bgzf_core.h (what bgzf_block_kernel runs per BGZF block) replayed on the host: the lanes of a workgroup as loops, the phases in launch order,
// the blocks one after the other through ONE workgroup's token region; then the gather (an exclusive scan of the sizes and a copy).
// Staging and token regions are sized exactly, so a sanitizer build sees any byte written past them.
// As a library (tests/test_host_bgzf.py) and, with BGZF_SIM_MAIN, as a stand-alone program for a sanitizer build:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DBGZF_SIM_MAIN -o bgzf_sim_asan bgzf_sim.cpp -lz && ./bgzf_sim_asan FILE...
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../moni_align_amd/csrc/bgzf_core.h"

static const uint8_t BGZF_EOF[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

extern "C" {

// out: room for len + 31 * blocks + 28 bytes.  stats: in_bytes, out_bytes, blocks, stored_blocks, matches, literals, bit-count mismatches.
// Returns MONI_OK / MONI_EINVAL as moni_bgzf_compress does.
int bgzfsim_compress(const uint8_t* text, uint64_t len, const moni_bgzf_params_t* prm, uint8_t* out, uint64_t* out_len, uint64_t* stats) {
    if (!prm || !out || !out_len || !bgzf_params_ok(*prm) || (!text && len)) return MONI_EINVAL;
    const uint64_t nb = (len + prm->block_size - 1) / prm->block_size;
    std::vector<uint32_t> staging((size_t)nb * (bgzf_slot_bytes(prm->block_size) / 4u), 0u), tok(nb ? BGZF_MAX_BLOCK : 0u);
    std::vector<uint64_t> blen(nb, 0), boff(nb, 0);
    unsigned long long counters[4] = {0, 0, 0, 0};
    // the text in a block of exactly len bytes: a read past the end is a read past the allocation
    std::unique_ptr<uint8_t[]> copy(new uint8_t[len ? len : 1]);
    if (len) memcpy(copy.get(), text, len);
    bgzf_args_t G;
    G.text = copy.get(); G.len = len; G.block_size = prm->block_size; G.level = prm->level; G.n_blocks = nb;
    G.staging = staging.data(); G.tok = tok.data(); G.out_len = blen.data(); G.out_off = boff.data(); G.counters = counters;
    std::unique_ptr<bgzf_shared_t> S(new bgzf_shared_t);
    for (uint64_t b = 0; b < nb; ++b) bgzf_block(*S, G, b, tok.data());
    uint64_t pos = 0;
    for (uint64_t b = 0; b < nb; ++b) {
        if (blen[b] > bgzf_slot_bytes(prm->block_size) || boff[b] != b * (bgzf_slot_bytes(prm->block_size) / 8u)) return MONI_ERANGE;
        memcpy(out + pos, reinterpret_cast<const uint8_t*>(staging.data()) + 8 * boff[b], blen[b]);
        pos += blen[b];
    }
    if (prm->eof) { memcpy(out + pos, BGZF_EOF, 28); pos += 28; }
    *out_len = pos;
    if (stats) {
        stats[0] = len; stats[1] = pos; stats[2] = nb + (prm->eof ? 1 : 0); stats[3] = counters[2]; stats[4] = counters[0]; stats[5] = counters[1];
        stats[6] = counters[3];
    }
    return MONI_OK;
}

// The code-length builder alone: freq[n] -> len[n], code[n] (bit-reversed); n <= 288, limit <= 15.
int bgzfsim_build_lengths(const uint32_t* freq, uint32_t n, uint32_t limit, int complete, uint8_t* len, uint16_t* code) {
    if (n > 288 || limit < 1 || limit > 15) return MONI_EINVAL;
    std::unique_ptr<bgzf_hl_t<288>> W(new bgzf_hl_t<288>);
    for (uint32_t l = 0; l < BGZF_T; ++l) bgzf_hl_rank(freq, n, len, W->A, W->sym, &W->nu, l);
    bgzf_hl_finish(n, limit, complete != 0, len, code, W->A, W->sym, W->nu, W->cnt, W->nxt);
    return MONI_OK;
}

// length / distance -> symbol, extra bits, extra value (out[3])
void bgzfsim_len_sym(uint32_t len, uint32_t* out) { bgzf_len_sym(len, out[0], out[1], out[2]); }
void bgzfsim_dist_sym(uint32_t dist, uint32_t* out) { bgzf_dist_sym(dist, out[0], out[1], out[2]); }
// the hash-table slot of three bytes
uint32_t bgzfsim_hash3(const uint8_t* p) { return bgzf_hash3(p); }
// crc(A B) from crc(A), crc(B) and |B|
uint32_t bgzfsim_crc_combine(uint32_t crc_a, uint32_t crc_b, uint32_t len_b) { return bgzf_crc_shift(crc_a, len_b) ^ crc_b; }

}  // extern "C"

#ifdef BGZF_SIM_MAIN
#include <zlib.h>

// every member of `z` inflated with zlib, the CRC and ISIZE of each checked; the concatenation must be `want`
static bool inflate_all(const std::vector<uint8_t>& z, const std::vector<uint8_t>& want) {
    std::vector<uint8_t> got;
    size_t at = 0;
    while (at < z.size()) {
        if (z.size() - at < 26) return false;
        const size_t total = (size_t)(z[at + 16] | (z[at + 17] << 8)) + 1;
        if (at + total > z.size()) return false;
        std::vector<uint8_t> buf(65536);
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, -15) != Z_OK) return false;
        zs.next_in = const_cast<uint8_t*>(z.data()) + at + 18; zs.avail_in = (uInt)(total - 26);
        zs.next_out = buf.data(); zs.avail_out = (uInt)buf.size();
        const int rc = inflate(&zs, Z_FINISH);
        const size_t n = zs.total_out;
        const bool used_all = zs.avail_in == 0;
        inflateEnd(&zs);
        if (rc != Z_STREAM_END || !used_all) return false;
        uint32_t crc, isize;
        memcpy(&crc, z.data() + at + total - 8, 4); memcpy(&isize, z.data() + at + total - 4, 4);
        if (isize != n || crc != (uint32_t)crc32(0, buf.data(), (uInt)n)) return false;
        got.insert(got.end(), buf.begin(), buf.begin() + n);
        at += total;
    }
    return got == want;
}

static int run_case(const char* what, const std::vector<uint8_t>& text, uint32_t block_size, uint32_t level) {
    moni_bgzf_params_t p = {block_size, level, 1, 0};
    const uint64_t nb = (text.size() + block_size - 1) / block_size;
    std::vector<uint8_t> out(text.size() + 31 * nb + 28);          // exactly the bound
    uint64_t n = 0, st[7];
    const int rc = bgzfsim_compress(text.data(), text.size(), &p, out.data(), &n, st);
    out.resize(n);
    const bool ok = rc == MONI_OK && st[6] == 0 && inflate_all(out, text);
    printf("%-28s %8zu bytes  block_size %5u level %u -> %8llu bytes, %llu blocks (%llu stored), %llu matches  %s\n", what, text.size(), block_size, level,
           (unsigned long long)n, (unsigned long long)st[2], (unsigned long long)st[3], (unsigned long long)st[4], ok ? "ok" : "FAILED");
    return ok ? 0 : 1;
}

int main(int argc, char** argv) {
    int bad = 0;
    uint64_t x = 88172645463325252ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (uint8_t)(x >> 32); };
    for (size_t len : {(size_t)0, (size_t)1, (size_t)2, (size_t)3, (size_t)1000, (size_t)65279, (size_t)65280, (size_t)65281}) {
        std::vector<uint8_t> a(len, 'A'), r(len), m(len);
        for (size_t i = 0; i < len; ++i) { r[i] = rnd(); m[i] = "ACGT\x00\xff"[rnd() % 6]; }
        for (uint32_t level : {1u, 0u}) { bad += run_case("runs", a, 65280, level); bad += run_case("random", r, 65280, level); bad += run_case("mixed", m, 65280, level); }
        bad += run_case("mixed, small blocks", m, 258, 1);
    }
    for (int i = 1; i < argc; ++i) {
        FILE* f = fopen(argv[i], "rb");
        if (!f) { fprintf(stderr, "cannot read %s\n", argv[i]); return 2; }
        std::vector<uint8_t> t;
        uint8_t buf[65536];
        size_t k;
        while ((k = fread(buf, 1, sizeof buf, f)) > 0) t.insert(t.end(), buf, buf + k);
        fclose(f);
        for (uint32_t bs : {65280u, 4096u, 258u, 3u, 1u}) bad += run_case(argv[i], t, bs, 1);
        bad += run_case(argv[i], t, 65280, 0);
    }
    printf("%d case(s) failed\n", bad);
    return bad ? 1 : 0;
}
#endif
