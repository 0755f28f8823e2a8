// Buf<Tp, Mem>: a grow-only block of Tp that owns its memory.  Mem says where the memory lives:
//   static void* alloc(size_t bytes)      nullptr when there is none
//   static void  free(void* p)
//   static size_t grown(size_t need)      elements to allocate when `need` are asked for (the slack that spares the next regrow)
//   static constexpr bool host_addressable   the host may memcpy it (ensure_keep)
// The library's two policies (device memory, pinned host memory) are in moni_hip.hip; the host tests bring a counting one.  Nothing here
// touches the HIP runtime.  A Buf must not have static storage duration: its destructor would call into a runtime that has shut down.
#pragma once
#include <cstddef>
#include <cstring>
#include <utility>

#include "../../include/moni_hip.h"

template <class Tp, class Mem>
struct Buf {
    Tp* p = nullptr;
    size_t cap = 0;                 // elements

    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~Buf() { release(); }

    void release() { if (p) Mem::free(p); p = nullptr; cap = 0; }

    // room for `need` elements; the contents are not kept.  The old block goes before the new one is asked for.
    int ensure(size_t need) { return need <= cap ? MONI_OK : alloc_exact(Mem::grown(need)); }

    // exactly `bytes` (a block of fixed size: no slack); cap counts the whole elements in it
    int alloc_bytes(size_t bytes) {
        release();
        p = static_cast<Tp*>(Mem::alloc(bytes));
        if (!p) return MONI_ENOMEM;
        cap = bytes / sizeof(Tp);
        return MONI_OK;
    }
    int alloc_exact(size_t n) { return alloc_bytes(n * sizeof(Tp)); }

    // room for exactly `exact_cap` elements with the first `keep_bytes` bytes kept: the new block first, then the copy, then the old
    // block goes.  When there is no memory the old block stays as it is.
    int ensure_keep(size_t exact_cap, size_t keep_bytes) {
        static_assert(Mem::host_addressable, "ensure_keep copies with memcpy");
        if (exact_cap <= cap) return MONI_OK;
        Tp* nb = static_cast<Tp*>(Mem::alloc(exact_cap * sizeof(Tp)));
        if (!nb) return MONI_ENOMEM;
        if (p && keep_bytes) memcpy(nb, p, keep_bytes);
        if (p) Mem::free(p);
        p = nb; cap = exact_cap;
        return MONI_OK;
    }
};
