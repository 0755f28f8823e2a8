// Buf<Tp, Mem> (moni_align_amd/csrc/owned_buf.hpp) over a malloc-backed policy that counts what is live and can be told to fail the next
// allocation.  Built with -fsanitize=address,undefined (tests/test_owned_buf.py): a double free, a leak at exit or a read past a block ends
// the run.  Prints OK.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "../../moni_align_amd/csrc/owned_buf.hpp"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "owned_buf_test: %s fails (line %d)\n", #x, __LINE__); exit(1); } } while (0)

static std::map<void*, size_t>* g_blocks;      // live blocks and their bytes (a pointer: built in main, gone before the counts are read for the last time)
static size_t g_bytes = 0, g_allocs = 0, g_frees = 0;
static bool g_fail_next = false;

template <int Variant>      // 0: the growth of the device buffers, 1: of the pinned ones
struct CountingMem {
    static constexpr bool host_addressable = true;
    static void* alloc(size_t bytes) {
        if (g_fail_next) { g_fail_next = false; return nullptr; }
        void* p = malloc(bytes ? bytes : 1);      // exactly what is asked for: the sanitizer sees any access beyond it
        CHECK(p);
        (*g_blocks)[p] = bytes; g_bytes += bytes; ++g_allocs;
        return p;
    }
    static void free(void* p) {
        auto it = g_blocks->find(p);
        CHECK(it != g_blocks->end());             // freed once, and only what alloc handed out
        g_bytes -= it->second; g_blocks->erase(it); ++g_frees;
        ::free(p);
    }
    static size_t grown(size_t need) { return Variant == 0 ? need + need / 8 + 64 : need + need / 4; }
};
template <class Tp> using DB = Buf<Tp, CountingMem<0>>;
template <class Tp> using HB = Buf<Tp, CountingMem<1>>;
static size_t live() { return g_blocks->size(); }

struct Pair { uint64_t x, y; };
struct Batch {      // the shape of the library's ResidentBatch
    DB<uint8_t> seq; DB<uint64_t> offs;
    uint64_t n_reads = 0, total_len = 0, max_len = 0;
    DB<Pair> blk; std::vector<Pair> h_blk;
    std::vector<uint8_t> h_seq; std::vector<uint64_t> h_offs;
};
static void fill(Batch& b, uint64_t n) {
    CHECK(b.seq.ensure(10 * n + 16) == MONI_OK && b.offs.ensure(n + 1) == MONI_OK && b.blk.ensure(n / 32 + 2) == MONI_OK);
    b.n_reads = n; b.total_len = 10 * n; b.max_len = 10;
    b.h_blk.assign(n / 32 + 2, Pair{n, n}); b.h_seq.assign(10 * n, (uint8_t)n); b.h_offs.assign(n + 1, n);
    b.seq.p[0] = (uint8_t)n;
}

int main() {
    std::map<void*, size_t> blocks;
    g_blocks = &blocks;

    {   // destruction frees; release() twice
        DB<uint32_t> a;
        CHECK(a.p == nullptr && a.cap == 0);
        CHECK(a.ensure(100) == MONI_OK && a.p && a.cap == 100 + 100 / 8 + 64 && live() == 1 && g_bytes == a.cap * 4);
        a.p[a.cap - 1] = 7;
        DB<uint32_t> b;
        CHECK(b.ensure(5) == MONI_OK && live() == 2);
        b.release();
        CHECK(b.p == nullptr && b.cap == 0 && live() == 1);
        b.release();
        CHECK(b.p == nullptr && b.cap == 0 && live() == 1 && g_frees == 1);
    }
    CHECK(live() == 0 && g_bytes == 0 && g_frees == 2);

    {   // the two growth formulas; no allocation while the need fits; the old block goes when it does not
        const size_t needs[5] = {0, 1, 7, 64, 1000};
        for (size_t n : needs) {
            DB<uint64_t> d; HB<uint64_t> h;
            const size_t a0 = g_allocs;
            CHECK(d.ensure(n) == MONI_OK && h.ensure(n) == MONI_OK);
            if (n == 0) { CHECK(d.p == nullptr && d.cap == 0 && h.p == nullptr && h.cap == 0 && g_allocs == a0); continue; }      // nothing asked for: nothing allocated
            CHECK(d.cap == n + n / 8 + 64 && h.cap == n + n / 4 && g_allocs == a0 + 2);
            CHECK(g_bytes == (d.cap + h.cap) * 8);
            uint64_t* const dp = d.p;
            CHECK(d.ensure(d.cap) == MONI_OK && d.ensure(1) == MONI_OK && d.ensure(0) == MONI_OK && d.p == dp && g_allocs == a0 + 2);
            const size_t f0 = g_frees, c0 = d.cap;
            CHECK(d.ensure(c0 + 1) == MONI_OK && d.cap == (c0 + 1) + (c0 + 1) / 8 + 64 && g_frees == f0 + 1 && live() == 2);
        }
        CHECK(DB<uint8_t>().ensure(0) == MONI_OK);
        DB<uint64_t> d; HB<uint64_t> h;
        CHECK(CountingMem<0>::grown(0) == 64 && CountingMem<0>::grown(1) == 65 && CountingMem<0>::grown(7) == 71 && CountingMem<0>::grown(64) == 136 && CountingMem<0>::grown(1000) == 1189);
        CHECK(CountingMem<1>::grown(0) == 0 && CountingMem<1>::grown(1) == 1 && CountingMem<1>::grown(7) == 8 && CountingMem<1>::grown(64) == 80 && CountingMem<1>::grown(1000) == 1250);
    }
    CHECK(live() == 0);

    {   // exact sizes: no slack
        DB<uint32_t> a;
        CHECK(a.alloc_exact(4) == MONI_OK && a.cap == 4 && g_bytes == 16);
        CHECK(a.alloc_bytes(8) == MONI_OK && a.cap == 2 && g_bytes == 8 && live() == 1);
        DB<Pair> t;
        CHECK(t.alloc_bytes(8) == MONI_OK && t.p && t.cap == 0 && live() == 2);      // a block smaller than an element is still owned
    }
    CHECK(live() == 0);

    {   // a failed ensure: {nullptr, 0}, the old block freed
        DB<uint32_t> a;
        CHECK(a.ensure(10) == MONI_OK && live() == 1);
        g_fail_next = true;
        CHECK(a.ensure(a.cap + 1) == MONI_ENOMEM && a.p == nullptr && a.cap == 0 && live() == 0);
        CHECK(a.ensure(10) == MONI_OK && live() == 1);      // and usable again
    }
    CHECK(live() == 0);

    {   // moves
        DB<uint32_t> a;
        CHECK(a.ensure(10) == MONI_OK);
        uint32_t* const ap = a.p; const size_t ac = a.cap;
        DB<uint32_t> b(std::move(a));
        CHECK(a.p == nullptr && a.cap == 0 && b.p == ap && b.cap == ac && live() == 1);
        DB<uint32_t> c;
        CHECK(c.ensure(20) == MONI_OK && live() == 2);
        const size_t f0 = g_frees;
        c = std::move(b);                                   // c's old block goes, once
        CHECK(b.p == nullptr && b.cap == 0 && c.p == ap && c.cap == ac && live() == 1 && g_frees == f0 + 1);
        DB<uint32_t>& self = c;
        c = std::move(self);                                // self-move: nothing happens
        CHECK(c.p == ap && c.cap == ac && live() == 1 && g_frees == f0 + 1);
        DB<uint32_t> d;
        CHECK(d.ensure(30) == MONI_OK);
        uint32_t* const dp = d.p; const size_t dc = d.cap;
        std::swap(c, d);
        CHECK(c.p == dp && c.cap == dc && d.p == ap && d.cap == ac && live() == 2 && g_frees == f0 + 1);
        DB<uint32_t> e;
        std::swap(e, d);                                    // with an empty one
        CHECK(e.p == ap && d.p == nullptr && d.cap == 0 && live() == 2);
    }
    CHECK(live() == 0);

    {   // structs of buffers: swap, a vector that reallocates, clear
        Batch x, y;
        fill(x, 40); fill(y, 7);
        uint8_t* const xs = x.seq.p; uint8_t* const ys = y.seq.p;
        CHECK(live() == 6);
        const size_t f0 = g_frees;
        std::swap(x, y);
        CHECK(x.seq.p == ys && y.seq.p == xs && x.n_reads == 7 && y.n_reads == 40 && x.h_offs.size() == 8 && y.h_offs.size() == 41 && x.h_seq[0] == 7 && y.blk.p && live() == 6 && g_frees == f0);
        std::vector<Batch> stash;
        stash.resize(1);
        std::swap(x, stash[0]);
        CHECK(x.seq.p == nullptr && x.n_reads == 0 && stash[0].seq.p == ys && live() == 6);
        const Batch* const at0 = stash.data();
        size_t n = 1;
        while (stash.data() == at0) stash.resize(++n);      // up across a reallocation: the elements move, nothing is freed or copied
        stash.resize(n + 100);
        CHECK(stash[0].seq.p == ys && stash[0].seq.p[0] == 7 && stash[0].n_reads == 7 && stash[0].h_seq.size() == 70 && stash[n].seq.p == nullptr && live() == 6 && g_frees == f0);
        fill(stash[n + 50], 3);
        CHECK(live() == 9);
        stash.clear();
        CHECK(live() == 3 && g_frees == f0 + 6);            // y is left
        CHECK(y.seq.p == xs && y.seq.p[0] == 40);
    }
    CHECK(live() == 0);

    {   // ensure_keep: the first keep_bytes survive, nothing beyond them is read, the old block goes after the copy; failure keeps the old block
        HB<char> o;
        CHECK(o.ensure_keep(16, 0) == MONI_OK && o.cap == 16 && g_bytes == 16);
        for (int i = 0; i < 16; ++i) o.p[i] = (char)('a' + i);
        char* const p0 = o.p;
        CHECK(o.ensure_keep(16, 16) == MONI_OK && o.ensure_keep(3, 0) == MONI_OK && o.p == p0 && live() == 1);      // it fits: nothing moves
        const size_t f0 = g_frees;
        CHECK(o.ensure_keep(100, 16) == MONI_OK && o.cap == 100 && g_bytes == 100 && live() == 1 && g_frees == f0 + 1);      // keep == the old block's size: one byte more would be past it
        for (int i = 0; i < 16; ++i) CHECK(o.p[i] == (char)('a' + i));
        CHECK(o.ensure_keep(1000, 5) == MONI_OK && o.cap == 1000 && live() == 1);
        for (int i = 0; i < 5; ++i) CHECK(o.p[i] == (char)('a' + i));
        char* const p1 = o.p;
        g_fail_next = true;
        CHECK(o.ensure_keep(5000, 5) == MONI_ENOMEM && o.p == p1 && o.cap == 1000 && o.p[4] == 'e' && live() == 1);
        HB<char> fresh;
        CHECK(fresh.ensure_keep(64, 0) == MONI_OK && fresh.cap == 64);                  // from nothing
        HB<char> fresh2;
        CHECK(fresh2.ensure_keep(64, 10) == MONI_OK && fresh2.cap == 64);               // nothing to keep from: nothing is read
    }
    CHECK(live() == 0 && g_bytes == 0 && g_allocs == g_frees);
    printf("OK %zu blocks allocated and freed\n", g_allocs);
    return 0;
}
