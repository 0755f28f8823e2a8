// inflate_core.h (what inflate_member_kernel runs per BGZF member) replayed on the host: the lanes of a wavefront as loops, the phases in
// launch order, the members one after the other through ONE workgroup's shared state; around it the walk over the members' headers that
// moni_bgzf_inflate does.  The input, the text and the tables are sized exactly, so a sanitizer build sees any byte touched past them.
// As a library (tests/test_host_inflate.py) and, with INFLATE_SIM_MAIN, as a stand-alone program for a sanitizer build:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DINFLATE_SIM_MAIN -o inflate_sim_asan inflate_sim.cpp -lz && ./inflate_sim_asan FILE...
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../moni_align_amd/csrc/inflate_core.h"

extern "C" {

int inflsim_scan(const uint8_t* d, uint64_t len, uint64_t* n_blocks, uint64_t* used, uint64_t* out_bytes) {
    if (!d && len) return MONI_EINVAL;
    uint64_t at = 0, nb = 0, ob = 0;
    int rc = 0;
    infl_member_t m;
    while (at < len && (rc = infl_member_at(d, len, at, m)) == 0) { at += m.pay_off + m.pay_len + 8u; nb += 1; ob += m.isize; }
    *n_blocks = nb; *used = at; *out_bytes = ob;
    return rc == 2 ? MONI_EINVAL : MONI_OK;
}

// out: room for out_cap bytes (the sum of ISIZE is enough).  stats: blocks, bad_blocks, first_bad_block, bad_reason, stored, fixed, dynamic.
// Returns MONI_OK / MONI_EINVAL as moni_bgzf_inflate does; MONI_ERANGE where out_cap is too small.
int inflsim_inflate(const uint8_t* data, uint64_t len, uint32_t check_crc, uint8_t* out, uint64_t out_cap, uint64_t* out_len, uint64_t* stats) {
    if (!out_len || !stats || check_crc > 1 || (!data && len)) return MONI_EINVAL;
    *out_len = 0;
    for (int i = 0; i < 7; ++i) stats[i] = 0;
    if (!len) return MONI_OK;
    uint64_t nb = 0, used = 0, ob = 0;
    const int scan = inflsim_scan(data, len, &nb, &used, &ob);
    // the members in a block of exactly `used` bytes: a read past the last member is a read past the allocation
    std::unique_ptr<uint8_t[]> in(new uint8_t[used ? used : 1]);
    memcpy(in.get(), data, used);
    std::vector<infl_member_t> mem(nb);
    uint64_t text = 0;
    for (uint64_t b = 0, at = 0; b < nb; ++b) {
        infl_member_at(in.get(), used, at, mem[b]);
        mem[b].out_off = text;
        text += infl_slot_bytes(mem[b].isize);
        at += mem[b].pay_off + mem[b].pay_len + 8u;
    }
    std::unique_ptr<uint8_t[]> slots(new uint8_t[text ? text : 1]);
    std::vector<uint32_t> status(nb, 0xFFFFFFFFu);
    unsigned long long counters[3] = {0, 0, 0};
    infl_args_t G;
    G.in = in.get(); G.mem = mem.data(); G.n_members = nb; G.out = slots.get(); G.status = status.data(); G.counters = counters; G.check_crc = check_crc;
    std::unique_ptr<infl_shared_t> S(new infl_shared_t);
    for (uint64_t b = 0; b < nb; ++b) infl_member(*S, G, b);
    uint64_t bad = 0, first_bad = 0;
    uint32_t reason = MONI_INF_OK;
    for (uint64_t b = nb; b-- > 0;)
        if (status[b] != MONI_INF_OK) { bad += 1; first_bad = b; reason = status[b]; }
    if (used < len) {
        if (!bad) { first_bad = nb; reason = scan == MONI_EINVAL ? MONI_INF_HEADER : MONI_INF_TRUNCATED; }
        bad += 1;
    }
    stats[0] = nb + (used < len ? 1 : 0); stats[1] = bad; stats[2] = first_bad; stats[3] = reason;
    stats[4] = counters[0]; stats[5] = counters[1]; stats[6] = counters[2];
    if (bad) return MONI_EINVAL;
    if (text > out_cap) return MONI_ERANGE;
    if (text) memcpy(out, slots.get(), text);
    *out_len = text;
    return MONI_OK;
}

}  // extern "C"

#ifdef INFLATE_SIM_MAIN
#include <zlib.h>

typedef std::vector<uint8_t> bytes_t;

// one BGZF member around the raw DEFLATE stream zlib makes of `text`
static bytes_t member(const bytes_t& text, int level, int strategy) {
    bytes_t z(text.size() + text.size() / 1000 + 128);
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    deflateInit2(&zs, level, Z_DEFLATED, -15, 9, strategy);
    zs.next_in = const_cast<uint8_t*>(text.data()); zs.avail_in = (uInt)text.size();
    zs.next_out = z.data(); zs.avail_out = (uInt)z.size();
    deflate(&zs, Z_FINISH);
    z.resize(zs.total_out);
    deflateEnd(&zs);
    const uint32_t total = 18u + (uint32_t)z.size() + 8u, crc = (uint32_t)crc32(0, text.data(), (uInt)text.size()), n = (uint32_t)text.size();
    bytes_t m = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)((total - 1) & 0xff), (uint8_t)((total - 1) >> 8)};
    m.insert(m.end(), z.begin(), z.end());
    for (int i = 0; i < 4; ++i) m.push_back((uint8_t)(crc >> (8 * i)));
    for (int i = 0; i < 4; ++i) m.push_back((uint8_t)(n >> (8 * i)));
    return m;
}

// the replay over `z`; where it says MONI_OK the text must be `want` (NULL: no text to hold it to)
static int run(const char* what, const bytes_t& z, const bytes_t* want, bool must_pass) {
    uint64_t nb, used, ob, n = 0, st[7];
    inflsim_scan(z.data(), z.size(), &nb, &used, &ob);
    bytes_t out((size_t)ob);          // exactly the sum of ISIZE
    const int rc = inflsim_inflate(z.data(), z.size(), 1, out.data(), out.size(), &n, st);
    bool ok = rc == MONI_OK ? (!want || (n == want->size() && (!n || !memcmp(out.data(), want->data(), n)))) : (rc == MONI_EINVAL && !must_pass && st[1] > 0);
    if (what) printf("%-30s %8zu bytes, %llu members -> rc %d, %llu bytes, bad %llu first %llu reason %llu, blocks %llu/%llu/%llu  %s\n", what, z.size(), (unsigned long long)st[0], rc,
           (unsigned long long)n, (unsigned long long)st[1], (unsigned long long)st[2], (unsigned long long)st[3], (unsigned long long)st[4], (unsigned long long)st[5],
           (unsigned long long)st[6], ok ? "ok" : "FAILED");
    return ok ? 0 : 1;
}

int main(int argc, char** argv) {
    int bad = 0;
    uint64_t x = 88172645463325252ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (uint32_t)(x >> 32); };
    unsigned long long damaged = 0, refused = 0;
    for (size_t len : {(size_t)0, (size_t)1, (size_t)2, (size_t)1000, (size_t)20000, (size_t)65280}) {
        bytes_t a(len, 'A'), r(len), m(len);
        for (size_t i = 0; i < len; ++i) { r[i] = (uint8_t)rnd(); m[i] = (uint8_t)"ACGTN#IIIFF:\n"[rnd() % 13]; }
        for (const bytes_t* t : {&a, &r, &m})
            for (int level : {0, 1, 6, 9})
                for (int strategy : {Z_DEFAULT_STRATEGY, Z_FIXED}) {
                    const bytes_t z = member(*t, level, strategy);
                    bad += run("zlib member", z, t, true);
                    // one byte changed, one byte dropped, the stream cut: whatever the replay answers, it stays inside its buffers, and
                    // where it answers MONI_OK (a flip in MTIME, say) the text is the original
                    for (size_t at = 0; at < z.size(); at += 1 + z.size() / 64) {
                        bytes_t f = z; f[at] ^= (uint8_t)(1u << (rnd() % 8));
                        bytes_t g = z; g.erase(g.begin() + at);
                        bytes_t h(z.begin(), z.begin() + at);
                        for (const bytes_t* v : {&f, &g, &h}) { ++damaged; uint64_t nb, used, ob, n = 0, st[7]; inflsim_scan(v->data(), v->size(), &nb, &used, &ob);
                            bytes_t out((size_t)ob); const int rc = inflsim_inflate(v->data(), v->size(), 1, out.data(), out.size(), &n, st);
                            if (rc == MONI_EINVAL) ++refused; else if (rc != MONI_OK || (v->size() && (n != t->size() || (n && memcmp(out.data(), t->data(), n))))) { ++bad; printf("damaged copy accepted with other text\n"); } }
                    }
                }
    }
    printf("%llu damaged copies, %llu refused\n", damaged, refused);
    for (int i = 1; i < argc; ++i) {          // FILE: a stream; FILE.want beside it, where the stream is good, its text
        FILE* f = fopen(argv[i], "rb");
        if (!f) { fprintf(stderr, "cannot read %s\n", argv[i]); return 2; }
        bytes_t z, w;
        uint8_t buf[65536];
        size_t k;
        while ((k = fread(buf, 1, sizeof buf, f)) > 0) z.insert(z.end(), buf, buf + k);
        fclose(f);
        const std::string wn = std::string(argv[i]) + ".want";
        FILE* g = fopen(wn.c_str(), "rb");
        if (g) { while ((k = fread(buf, 1, sizeof buf, g)) > 0) w.insert(w.end(), buf, buf + k); fclose(g); }
        bad += run(argv[i], z, g ? &w : nullptr, g != nullptr);
    }
    printf("%d case(s) failed\n", bad);
    return bad ? 1 : 0;
}
#endif
