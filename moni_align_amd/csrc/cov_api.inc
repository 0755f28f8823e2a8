// Host side of the depth of coverage (included inside extern "C" of moni_hip.hip, behind bamin_api.inc): the kernels are in cov_kernels.hip.
// An add = cov_check_kernel (the record check of the sort unless the records come from it, the classes' counts), the reservation of the
// counted records against the object's 2^31, cov_add_kernel.  The seal = rocPRIM's inclusive scan of the slots in place - as 32-bit unsigned
// words, so no partial sum overflows - and cov_reduce_kernel.  A piece of text = cov_tail_kernel, a scan, cov_compact_kernel, cov_len_kernel,
// a scan, cov_render_kernel.  The slots, the dictionary and the figures belong to the object; what a call needs beside them is the context's
// own (moni_ctx::cov), grow-only: the resident batch and every earlier result stay as they are.

struct moni_cov {
    int device = 0;
    uint32_t n_ref = 0;
    uint64_t S = 0;
    moni_cov_params_t prm = {};
    DBuf<int32_t> slots; DBuf<uint64_t> base; DBuf<uint8_t> names; DBuf<uint32_t> name_off; DBuf<moni_cov_ref_t> refs;
    std::vector<uint64_t> h_base; std::vector<moni_cov_ref_t> h_refs;
    std::atomic<uint64_t> counted{0};
    std::atomic<bool> sealed{false};
    uint64_t cursor = 0, carry = 0;          // moni_cov_next: the first slot not looked at yet; the slot behind the last line written
    bool done = false;
};

struct CovWiden { __host__ __device__ uint32_t operator()(uint8_t v) const { return v; } };

void moni_cov_params_default(moni_cov_params_t* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->exclude_flags = 0x704u;
}

int moni_cov_create(moni_ctx_t* c, const moni_cov_params_t* prm, moni_cov_t** out) {
    if (!c || !prm || !out || !c->bam.has_header || prm->reserved[0] || prm->reserved[1]) return MONI_EINVAL;
    HIPCHK(hipSetDevice(c->idx->device));
    moni_cov* v = new (std::nothrow) moni_cov;
    if (!v) return MONI_ENOMEM;
    v->device = c->idx->device; v->prm = *prm;
    // the dictionary, from the BAM header that moni_bam_set_header made: magic, l_text, the text, n_ref, then l_name, name, NUL, l_ref
    const std::vector<uint8_t>& H = c->bam.header;
    auto get32 = [&](size_t at) { return bam_get32(H.data() + at); };
    size_t at = 8 + (size_t)get32(4);
    v->n_ref = get32(at); at += 4;
    std::vector<uint8_t> names; std::vector<uint32_t> name_off(1, 0u);
    v->h_base.assign(1, 0ull);
    for (uint32_t r = 0; r < v->n_ref; ++r) {
        const uint32_t l_name = get32(at);
        names.insert(names.end(), H.begin() + (ptrdiff_t)(at + 4), H.begin() + (ptrdiff_t)(at + 4 + l_name - 1));
        name_off.push_back((uint32_t)names.size());
        const uint32_t ln = get32(at + 4 + l_name);
        moni_cov_ref_t f = {ln, 0, 0, 0};
        v->h_refs.push_back(f);
        v->h_base.push_back(v->h_base.back() + ln + 1u);
        at += 8 + (size_t)l_name;
    }
    v->S = v->h_base.back();
    int rc;
    if ((rc = v->slots.alloc_exact(v->S + 1)) || (rc = v->base.alloc_exact(v->h_base.size())) || (rc = v->names.alloc_exact(names.size() + 1)) ||
        (rc = v->name_off.alloc_exact(name_off.size())) || (rc = v->refs.alloc_exact(v->n_ref + 1))) { delete v; return refused(rc); }
    if (hipMemsetAsync(v->slots.p, 0, (v->S + 1) * sizeof(int32_t), c->stream) != hipSuccess ||
        hipMemcpyAsync(v->base.p, v->h_base.data(), v->h_base.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        (!names.empty() && hipMemcpyAsync(v->names.p, names.data(), names.size(), hipMemcpyHostToDevice, c->stream) != hipSuccess) ||
        hipMemcpyAsync(v->name_off.p, name_off.data(), name_off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) { delete v; return MONI_ENODEV; }
    *out = v;
    return MONI_OK;
}

void moni_cov_destroy(moni_cov_t* v) {
    if (!v) return;
    (void)hipSetDevice(v->device);
    delete v;
}

void moni_cov_test_set_counted(moni_cov_t* v, uint64_t counted) {
    if (v) v->counted.store(counted);
}

// rec[0, len) and off[0, n] are on the device.  The stream is synchronised when it returns.
static int cov_add_device(moni_ctx_t* c, moni_cov* v, const uint8_t* rec, uint64_t len, const uint64_t* off, uint64_t n, bool trusted, moni_cov_stats_t& st) {
    auto& V = c->cov;
    int rc;
    if ((rc = V.ctr.ensure(8)) || (rc = V.h_ctr.ensure(8))) return rc;
    if (!n) return MONI_OK;
    for (Event* e : {&V.e0, &V.e1, &V.e2, &V.e3})
        if (!e->h) HIPCHK(hipEventCreate(&e->h));
    cov_args_t G;
    memset(&G, 0, sizeof G);
    G.rec = rec; G.len = len; G.off = off; G.n = n; G.n_ref = v->n_ref; G.exclude = v->prm.exclude_flags; G.min_mapq = v->prm.min_mapq; G.trusted = trusted ? 1u : 0u;
    G.base = v->base.p; G.slots = v->slots.p; G.ctr = V.ctr.p;
    const dim3 lanes((unsigned)((n + COV_T - 1) / COV_T));
    HIPCHK(hipMemsetAsync(V.ctr.p, 0, 8 * sizeof(unsigned long long), c->stream));
    HIPCHK(hipMemsetAsync(V.ctr.p + 1, 0xFF, sizeof(unsigned long long), c->stream));
    HIPCHK(hipEventRecord(V.e0, c->stream));
    hipLaunchKernelGGL(cov_check_kernel, lanes, dim3(COV_T), 0, c->stream, G);
    HIPCHK(hipEventRecord(V.e1, c->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(V.h_ctr.p, V.ctr.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (V.h_ctr.p[0]) {          // before the pass that trusts the records
        st.bad_records = V.h_ctr.p[0]; st.first_bad_record = V.h_ctr.p[1] >> 8; st.bad_reason = (uint32_t)(V.h_ctr.p[1] & 0xFFu);
        return MONI_EINVAL;
    }
    const uint64_t counted = V.h_ctr.p[2 + COV_COUNTED];
    for (uint64_t have = v->counted.load();;) {          // the records of this call, or none of them
        if (have + counted >= COV_LIMIT) return MONI_ERANGE;
        if (v->counted.compare_exchange_weak(have, have + counted)) break;
    }
    st.counted = counted; st.unplaced = V.h_ctr.p[2 + COV_UNPLACED]; st.skipped_flag = V.h_ctr.p[2 + COV_FLAG]; st.skipped_mapq = V.h_ctr.p[2 + COV_MAPQ];
    HIPCHK(hipEventRecord(V.e2, c->stream));
    hipLaunchKernelGGL(cov_add_kernel, lanes, dim3(COV_T), 0, c->stream, G);
    HIPCHK(hipEventRecord(V.e3, c->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(V.h_ctr.p, V.ctr.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    st.clipped = V.h_ctr.p[6]; st.blocks = V.h_ctr.p[7];
    float a = 0, b = 0;
    HIPCHK(hipEventElapsedTime(&a, V.e0, V.e1)); HIPCHK(hipEventElapsedTime(&b, V.e2, V.e3));
    st.t_add = (a + b) * 1e-3;
    return MONI_OK;
}

// what both adds ask of their arguments; the device is set
static int cov_add_ready(moni_ctx_t* c, moni_cov* v) {
    if (!c || !v || !c->bam.has_header || c->idx->device != v->device || c->bam.dict.n_ref != v->n_ref || v->sealed.load()) return MONI_EINVAL;
    HIPCHK(hipSetDevice(c->idx->device));
    return MONI_OK;
}

int moni_cov_add(moni_ctx_t* c, moni_cov_t* v, const void* records, uint64_t len, const uint64_t* offs, uint64_t n, moni_cov_stats_t* stats) {
    int rc = cov_add_ready(c, v);
    if (rc || (!records && len) || (!offs && n)) return rc ? rc : MONI_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    auto& V = c->cov;
    moni_cov_stats_t st;
    memset(&st, 0, sizeof st);
    st.records = n;
    if ((n ? offs[n] : 0) != len || n >= (1ull << 32)) { st.bad_records = 1; st.first_bad_record = n; st.bad_reason = MONI_BAMSORT_LENGTH; rc = MONI_EINVAL; }
    else if ((rc = V.in.ensure(len + 8)) == MONI_OK && (rc = V.in_off.ensure(n + 1)) == MONI_OK && n) {
        HIPCHK(hipMemcpyAsync(V.in.p, records, len, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(V.in_off.p, offs, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        rc = cov_add_device(c, v, V.in.p, len, V.in_off.p, n, false, st);
    }
    st.t_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = st;
    return rc;
}

int moni_cov_add_sorted(moni_ctx_t* c, moni_cov_t* v, moni_cov_stats_t* stats) {
    int rc = cov_add_ready(c, v);
    if (rc || !c->bsort.have_sorted) return rc ? rc : MONI_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    moni_cov_stats_t st;
    memset(&st, 0, sizeof st);
    st.records = c->bsort.sorted_n;
    rc = cov_add_device(c, v, c->bsort.out.p, c->bsort.sorted_len, c->bsort.out_off.p, c->bsort.sorted_n, true, st);
    st.t_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = st;
    return rc;
}

int moni_cov_seal(moni_ctx_t* c, moni_cov_t* v, const moni_cov_ref_t** refs, uint32_t* n_ref) {
    if (!c || !v || !refs || !n_ref || c->idx->device != v->device) return MONI_EINVAL;
    HIPCHK(hipSetDevice(c->idx->device));
    if (!v->sealed.load() && v->n_ref) {
        // Every block adds its +1 and its -1 to slots of one reference, so the slots of a reference sum to zero and the scan starts every
        // reference at zero by itself.  On unsigned words: a partial sum is a difference of two depths and wraps harmlessly.
        uint32_t* w = reinterpret_cast<uint32_t*>(v->slots.p);
        size_t tmp_bytes = 0;
        if (rocprim::inclusive_scan(nullptr, tmp_bytes, w, w, (size_t)v->S, rocprim::plus<uint32_t>(), c->stream) != hipSuccess) return MONI_ENODEV;
        int rc = c->cov.scan_tmp.ensure(tmp_bytes + 16);
        if (rc) return rc;
        if (rocprim::inclusive_scan(c->cov.scan_tmp.p, tmp_bytes, w, w, (size_t)v->S, rocprim::plus<uint32_t>(), c->stream) != hipSuccess) return MONI_ENODEV;
        for (moni_cov_ref_t& f : v->h_refs) { f.bases = 0; f.min = 0xFFFFFFFFu; f.max = 0; }
        HIPCHK(hipMemcpyAsync(v->refs.p, v->h_refs.data(), v->n_ref * sizeof(moni_cov_ref_t), hipMemcpyHostToDevice, c->stream));
        const uint64_t per_group = (uint64_t)COV_T * COV_STEPS;
        hipLaunchKernelGGL(cov_reduce_kernel, dim3((unsigned)((v->S + per_group - 1) / per_group)), dim3(COV_T), 0, c->stream, v->slots.p, v->base.p, v->n_ref, v->S, v->refs.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(v->h_refs.data(), v->refs.p, v->n_ref * sizeof(moni_cov_ref_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    v->sealed.store(true);
    *refs = v->h_refs.data(); *n_ref = v->n_ref;
    return MONI_OK;
}

int moni_cov_next(moni_ctx_t* c, moni_cov_t* v, uint64_t max_bases, uint64_t max_lines, const char** text, uint64_t* len, int* done) {
    if (!c || !v || !text || !len || !done || !max_bases || !max_lines || !v->sealed.load() || c->idx->device != v->device) return MONI_EINVAL;
    HIPCHK(hipSetDevice(c->idx->device));
    auto& V = c->cov;
    int rc;
    if ((rc = V.h_text.ensure(1)) || (rc = V.h_ctr.ensure(8))) return rc;
    *text = V.h_text.p; *len = 0; *done = 1;
    if (v->done || v->cursor >= v->S) { v->done = true; return MONI_OK; }
    const uint64_t x0 = v->cursor, w = std::min(std::min(max_bases, (uint64_t)COV_MAX_CALL), v->S - x0);
    if ((rc = V.flag.ensure(w + 1)) || (rc = V.scan.ensure(w + 1))) return rc;
    covtext_args_t T;
    memset(&T, 0, sizeof T);
    T.depth = v->slots.p; T.base = v->base.p; T.n_ref = v->n_ref; T.S = v->S; T.x0 = x0; T.w = w; T.flag = V.flag.p; T.scan = V.scan.p; T.carry = v->carry;
    T.names = v->names.p; T.name_off = v->name_off.p;
    auto grid = [](uint64_t lanes) { return dim3((unsigned)((lanes + COV_T - 1) / COV_T)); };
    hipLaunchKernelGGL(cov_tail_kernel, grid(w + 1), dim3(COV_T), 0, c->stream, T);
    {
        auto in = rocprim::make_transform_iterator(V.flag.p, CovWiden());
        size_t tmp_bytes = 0;
        if (rocprim::exclusive_scan(nullptr, tmp_bytes, in, V.scan.p, 0u, (size_t)(w + 1), rocprim::plus<uint32_t>(), c->stream) != hipSuccess) return MONI_ENODEV;
        if ((rc = V.scan_tmp.ensure(tmp_bytes + 16))) return rc;
        if (rocprim::exclusive_scan(V.scan_tmp.p, tmp_bytes, in, V.scan.p, 0u, (size_t)(w + 1), rocprim::plus<uint32_t>(), c->stream) != hipSuccess) return MONI_ENODEV;
    }
    HIPCHK(hipGetLastError());
    V.h_ctr.p[0] = 0;
    HIPCHK(hipMemcpyAsync(V.h_ctr.p, V.scan.p + w, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const uint64_t ends = V.h_ctr.p[0] & 0xFFFFFFFFull, lines = std::min(ends, max_lines);
    uint64_t next = x0 + w;
    if (lines) {
        if ((rc = V.pos.ensure(lines)) || (rc = V.len.ensure(lines + 1)) || (rc = V.off.ensure(lines + 1))) return rc;
        T.pos = V.pos.p; T.lines = lines; T.len = V.len.p; T.off = V.off.p;
        hipLaunchKernelGGL(cov_compact_kernel, grid(w), dim3(COV_T), 0, c->stream, T);
        hipLaunchKernelGGL(cov_len_kernel, grid(lines + 1), dim3(COV_T), 0, c->stream, T);
        if ((rc = exclusive_scan_u64(c, V.len.p, V.off.p, lines + 1))) return rc;
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(V.h_ctr.p + 1, V.off.p + lines, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(V.h_ctr.p + 2, V.pos.p + (lines - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        const uint64_t bytes = V.h_ctr.p[1], last = V.h_ctr.p[2];
        if ((rc = V.text.ensure(bytes + 1)) || (rc = V.h_text.ensure(bytes + 1))) return rc;
        T.text = V.text.p;
        hipLaunchKernelGGL(cov_render_kernel, grid(lines), dim3(COV_T), 0, c->stream, T);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(V.h_text.p, V.text.p, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        *text = V.h_text.p; *len = bytes;
        v->carry = last + 1;
        if (ends > max_lines) next = last + 1;          // the run ends behind it are the next call's
    }
    // a reference's last slot holds no base: the call that would see nothing else is spared
    if (next < v->S && *std::upper_bound(v->h_base.begin(), v->h_base.end(), next) == next + 1) ++next;
    v->cursor = next;
    v->done = next >= v->S;
    *done = v->done ? 1 : 0;
    return MONI_OK;
}

int moni_cov_windows(moni_ctx_t* c, moni_cov_t* v, uint32_t ref_id, uint32_t window, const uint64_t** sums, uint64_t* n) {
    if (!c || !v || !sums || !n || !v->sealed.load() || c->idx->device != v->device || ref_id >= v->n_ref || window < 1u || window >= (1u << 31)) return MONI_EINVAL;
    HIPCHK(hipSetDevice(c->idx->device));
    auto& V = c->cov;
    const uint64_t ln = v->h_refs[ref_id].length, n_win = (ln + window - 1) / window;
    int rc;
    if ((rc = V.sums.ensure(n_win)) || (rc = V.h_sums.ensure(n_win))) return rc;
    const uint32_t per_lane = window < COV_W ? 1u : 0u;
    const uint64_t lanes = per_lane ? n_win : n_win * COV_W;
    hipLaunchKernelGGL(cov_window_kernel, dim3((unsigned)((lanes + COV_T - 1) / COV_T)), dim3(COV_T), 0, c->stream, v->slots.p + v->h_base[ref_id], ln, window, n_win, per_lane, V.sums.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(V.h_sums.p, V.sums.p, n_win * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *sums = V.h_sums.p; *n = n_win;
    return MONI_OK;
}
