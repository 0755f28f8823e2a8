// cov_core.h (what the kernels of the depth of coverage run per record, slot, line and window) replayed on the host: the lanes as loops, the
// passes in the order cov_api.inc launches them - an add: the check pass, the reservation, the add pass; the seal: the scan, the reduce with
// its wavefronts of COV_W lanes; a piece of text: the run-end flags, their scan, the compaction, the lengths, their scan, the render - and
// the iterator's carry exactly as moni_cov_next keeps it.  Every pass takes its elements LAST TO FIRST, so a later bad record is met before
// an earlier one.  The buffers are sized exactly, so a sanitizer build sees any byte read or written past them.
// As a library (tests/test_host_coverage.py) and, with COVERAGE_SIM_MAIN, as a stand-alone program for a sanitizer build:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DCOVERAGE_SIM_MAIN -o coverage_sim_asan coverage_sim.cpp && ./coverage_sim_asan
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../moni_align_amd/csrc/cov_core.h"

struct CovSim {
    uint32_t n_ref = 0, exclude = 0, min_mapq = 0;
    uint64_t S = 0, counted = 0, cursor = 0, carry = 0;
    bool sealed = false, done = false;
    std::vector<uint64_t> base;
    std::vector<uint8_t> names;
    std::vector<uint32_t> name_off;
    std::unique_ptr<int32_t[]> slots;          // exactly S
    std::vector<moni_cov_ref_t> refs;
    std::vector<char> text;
    std::vector<uint64_t> sums;
};

extern "C" {

void* covsim_create(const uint64_t* ln, uint32_t n_ref, const uint8_t* names, const uint32_t* name_off, uint32_t exclude, uint32_t min_mapq) {
    CovSim* v = new CovSim;
    v->n_ref = n_ref; v->exclude = exclude; v->min_mapq = min_mapq;
    v->base.assign(1, 0);
    for (uint32_t r = 0; r < n_ref; ++r) { v->base.push_back(v->base.back() + ln[r] + 1u); v->refs.push_back(moni_cov_ref_t{ln[r], 0, 0, 0}); }
    v->S = v->base.back();
    v->names.assign(names, names + name_off[n_ref]);
    v->name_off.assign(name_off, name_off + n_ref + 1);
    v->slots.reset(new int32_t[v->S ? v->S : 1]());
    return v;
}
void covsim_destroy(void* h) { delete static_cast<CovSim*>(h); }
void covsim_set_counted(void* h, uint64_t c) { static_cast<CovSim*>(h)->counted = c; }
const int32_t* covsim_slots(void* h) { return static_cast<CovSim*>(h)->slots.get(); }

// stats: records, counted, skipped_flag, skipped_mapq, unplaced, clipped, blocks, bad_records, first_bad_record, bad_reason
int covsim_add(void* h, const uint8_t* rec, uint64_t len, const uint64_t* off, uint64_t n, uint32_t trusted, uint64_t* stats) {
    CovSim* v = static_cast<CovSim*>(h);
    if (!v || !stats || (!rec && len) || (!off && n) || v->sealed) return MONI_EINVAL;
    memset(stats, 0, 10 * sizeof(uint64_t));
    stats[0] = n;
    if ((n ? off[n] : 0) != len) { stats[7] = 1; stats[8] = n; stats[9] = MONI_BAMSORT_LENGTH; return MONI_EINVAL; }
    if (!n) return MONI_OK;
    std::unique_ptr<uint8_t[]> r(new uint8_t[len ? len : 1]);          // exactly len bytes
    memcpy(r.get(), rec, len);
    uint64_t cls[4] = {0, 0, 0, 0}, bad = 0, first = ~0ull;
    for (uint64_t i = n; i-- > 0;) {
        const uint32_t c = cov_check(r.get(), len, off, i, v->n_ref, v->exclude, v->min_mapq, trusted != 0u);
        if (c >> 8) { ++bad; first = std::min(first, i << 8 | (c >> 8)); }
        else ++cls[c];
    }
    if (bad) { stats[7] = bad; stats[8] = first >> 8; stats[9] = first & 0xFFu; return MONI_EINVAL; }
    if (v->counted + cls[COV_COUNTED] >= COV_LIMIT) return MONI_ERANGE;
    v->counted += cls[COV_COUNTED];
    stats[1] = cls[COV_COUNTED]; stats[2] = cls[COV_FLAG]; stats[3] = cls[COV_MAPQ]; stats[4] = cls[COV_UNPLACED];
    int32_t* slots = v->slots.get();
    const uint64_t S = v->S;
    for (uint64_t i = n; i-- > 0;) {
        const uint8_t* q = r.get() + off[i];
        if (cov_class(q, v->exclude, v->min_mapq) != COV_COUNTED) continue;
        const uint32_t got = cov_blocks(q, v->base.data(), [&](uint64_t at, int d) { if (at >= S) abort(); slots[at] += d; });
        stats[5] += got >> 31; stats[6] += got & 0x7FFFFFFFu;
    }
    return MONI_OK;
}

int covsim_seal(void* h, moni_cov_ref_t* out) {
    CovSim* v = static_cast<CovSim*>(h);
    if (!v || !out) return MONI_EINVAL;
    if (!v->sealed && v->n_ref) {
        uint32_t run = 0;          // one scan over all slots, no restart: on unsigned words, as the device's
        for (uint64_t x = 0; x < v->S; ++x) { run += (uint32_t)v->slots[x]; v->slots[x] = (int32_t)run; }
        for (moni_cov_ref_t& f : v->refs) { f.bases = 0; f.min = 0xFFFFFFFFu; f.max = 0; }
        auto flush = [&](const cov_acc_t& a) {
            if (a.mn > a.mx) return;
            moni_cov_ref_t& f = v->refs[a.ref];
            f.bases += a.sum; f.min = std::min(f.min, a.mn); f.max = std::max(f.max, a.mx);
        };
        const uint64_t per_wave = (uint64_t)COV_W * COV_STEPS, n_waves = (v->S + per_wave - 1) / per_wave;
        for (uint64_t w = n_waves; w-- > 0;) {
            cov_acc_t a[COV_W];
            for (uint32_t l = 0; l < COV_W; ++l) cov_reduce(v->slots.get(), v->base.data(), v->n_ref, v->S, w * per_wave + l, a[l], flush);
            bool uniform = true;
            for (uint32_t l = 1; l < COV_W; ++l) uniform = uniform && a[l].ref == a[0].ref;
            if (uniform) {
                for (uint32_t l = 1; l < COV_W; ++l) { a[0].sum += a[l].sum; a[0].mn = std::min(a[0].mn, a[l].mn); a[0].mx = std::max(a[0].mx, a[l].mx); }
                flush(a[0]);
            } else
                for (uint32_t l = 0; l < COV_W; ++l) flush(a[l]);
        }
    }
    v->sealed = true;
    if (v->n_ref) memcpy(out, v->refs.data(), v->n_ref * sizeof(moni_cov_ref_t));
    return MONI_OK;
}

int covsim_next(void* h, uint64_t max_bases, uint64_t max_lines, const char** text, uint64_t* len, int* done) {
    CovSim* v = static_cast<CovSim*>(h);
    if (!v || !text || !len || !done || !max_bases || !max_lines || !v->sealed) return MONI_EINVAL;
    v->text.clear();
    *text = nullptr; *len = 0; *done = 1;
    if (v->done || v->cursor >= v->S) { v->done = true; return MONI_OK; }
    const uint64_t x0 = v->cursor, w = std::min(std::min(max_bases, (uint64_t)COV_MAX_CALL), v->S - x0);
    const int32_t* depth = v->slots.get();
    const uint64_t* base = v->base.data();
    std::unique_ptr<uint8_t[]> flag(new uint8_t[w + 1]);
    std::unique_ptr<uint32_t[]> scan(new uint32_t[w + 1]);
    for (uint64_t i = w + 1; i-- > 0;) {
        const uint64_t first = x0 + (i & ~(uint64_t)(COV_W - 1u));
        flag[i] = i < w ? (uint8_t)cov_tail(depth, base, cov_ref_from(base, cov_ref_of(base, v->n_ref, first), x0 + i), x0 + i) : (uint8_t)0;
    }
    uint32_t run = 0;
    for (uint64_t i = 0; i <= w; ++i) { scan[i] = run; run += flag[i]; }
    const uint64_t ends = scan[w], lines = std::min(ends, max_lines);
    uint64_t next = x0 + w;
    if (lines) {
        std::unique_ptr<uint64_t[]> pos(new uint64_t[lines]), ln(new uint64_t[lines + 1]), off(new uint64_t[lines + 1]);
        for (uint64_t i = w; i-- > 0;)
            if (flag[i] && scan[i] < lines) pos[scan[i]] = x0 + i;
        for (uint64_t k = lines + 1; k-- > 0;) ln[k] = k < lines ? cov_line_len(cov_line(depth, base, v->n_ref, pos.get(), k, v->carry), v->name_off.data()) : 0u;
        uint64_t at = 0;
        for (uint64_t k = 0; k <= lines; ++k) { off[k] = at; at += ln[k]; }
        const uint64_t bytes = off[lines], last = pos[lines - 1];
        std::unique_ptr<uint8_t[]> out(new uint8_t[bytes]);          // exactly the text's bytes
        memset(out.get(), 0xEE, bytes);
        for (uint64_t k = lines; k-- > 0;)
            cov_put_line(out.get() + off[k], cov_line(depth, base, v->n_ref, pos.get(), k, v->carry), v->names.data(), v->name_off.data());
        v->text.assign(out.get(), out.get() + bytes);
        v->carry = last + 1;
        if (ends > max_lines) next = last + 1;
    }
    if (next < v->S && *std::upper_bound(v->base.begin(), v->base.end(), next) == next + 1) ++next;
    v->cursor = next;
    v->done = next >= v->S;
    *text = v->text.data(); *len = v->text.size(); *done = v->done ? 1 : 0;
    return MONI_OK;
}

int covsim_windows(void* h, uint32_t ref_id, uint32_t window, const uint64_t** sums, uint64_t* n) {
    CovSim* v = static_cast<CovSim*>(h);
    if (!v || !sums || !n || !v->sealed || ref_id >= v->n_ref || window < 1u || window >= (1u << 31)) return MONI_EINVAL;
    const uint64_t ln = v->refs[ref_id].length, n_win = (ln + window - 1) / window;
    const int32_t* depth = v->slots.get() + v->base[ref_id];
    v->sums.assign(n_win, 0);
    for (uint64_t k = n_win; k-- > 0;) {
        const uint64_t lo = k * window, hi = std::min(lo + window, ln);
        if (window < COV_W) v->sums[k] = cov_window(depth, lo, hi, 0u, 1u);
        else for (uint32_t l = 0; l < COV_W; ++l) v->sums[k] += cov_window(depth, lo, hi, l, COV_W);
    }
    *sums = v->sums.data(); *n = n_win;
    return MONI_OK;
}

}  // extern "C"

#ifdef COVERAGE_SIM_MAIN
// a small run of every pass for a sanitizer build: three references, records at their edges, the text at the smallest windows
static std::vector<uint8_t> make(int32_t ref, int32_t pos, std::vector<uint32_t> ops, uint32_t flag) {
    std::vector<uint8_t> r(36 + 2 + 4 * ops.size() + 3, 0);
    auto put32 = [&](size_t at, uint32_t x) { for (int k = 0; k < 4; ++k) r[at + k] = (uint8_t)(x >> (8 * k)); };
    put32(0, (uint32_t)r.size() - 4); put32(4, (uint32_t)ref); put32(8, (uint32_t)pos);
    r[12] = 2; r[13] = 30; r[16] = (uint8_t)ops.size(); r[18] = (uint8_t)flag; r[19] = (uint8_t)(flag >> 8); r[36] = 'q';
    for (size_t k = 0; k < ops.size(); ++k) put32(38 + 4 * k, ops[k]);
    return r;
}
int main() {
    const uint64_t ln[3] = {1, 70, 200};
    const uint8_t names[] = "achrBc";
    const uint32_t name_off[4] = {0, 1, 5, 6};
    std::vector<std::vector<uint8_t>> recs = {make(0, 0, {3u << 4}, 0), make(1, 65, {10u << 4}, 0), make(1, 69, {1u << 4, 5u << 4 | 3u, 2u << 4}, 16),
                                              make(2, 199, {1u << 4}, 0), make(2, 0, {200u << 4}, 0x800), make(-1, -1, {}, 4), make(2, 5, {4u << 4}, 0x400)};
    std::vector<uint8_t> all; std::vector<uint64_t> off(1, 0);
    for (auto& r : recs) { all.insert(all.end(), r.begin(), r.end()); off.push_back(all.size()); }
    std::string whole;
    for (uint64_t mb : {1ull, 7ull, 1ull << 20})
        for (uint64_t ml : {1ull, 2ull, 1ull << 20}) {
            void* h = covsim_create(ln, 3, names, name_off, 0x704, 0);
            uint64_t st[10];
            if (covsim_add(h, all.data(), all.size(), off.data(), recs.size(), 0, st)) return 1;
            moni_cov_ref_t refs[3];
            if (covsim_seal(h, refs)) return 1;
            std::string text; const char* t; uint64_t l; int done = 0;
            while (!done) { if (covsim_next(h, mb, ml, &t, &l, &done)) return 1; text.append(t ? t : "", l); }
            if (whole.empty()) whole = text;
            if (text != whole) { fprintf(stderr, "the text depends on the window\n"); return 1; }
            const uint64_t* s; uint64_t n;
            for (uint32_t w : {1u, 16u, 70u, 1000u}) if (covsim_windows(h, 2, w, &s, &n)) return 1;
            covsim_destroy(h);
        }
    fputs(whole.c_str(), stdout);
    return 0;
}
#endif
