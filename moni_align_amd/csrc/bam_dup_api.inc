// Host side of duplicate marking (included inside extern "C" of moni_hip.hip, behind bam_sort_api.inc): the kernels are in bam_dup_kernels.hip.
// A run = bam_dupsig_kernel (checks, scores, end codes), bam_dupinv_kernel (where every record landed in the sort), bam_dupunit_kernel twice
// around a scan (the entries, compact, in input order).  The resolve = bam_dupprep_kernel, three stable radix sorts of the pairs (least
// significant key first: kind and score, k2, k1) and two of the ends (class and score, e), a key kernel between two passes, and the two flag
// kernels.  All buffers are the context's own (moni_ctx::bdup), grow-only.

static void bam_dup_bad(moni_ctx_t* c, moni_bam_run_dup_stats_t& ds) {
    auto& D = c->bdup;
    ds.run.bad_records = D.h_ctr.p[0]; ds.run.first_bad_record = D.h_ctr.p[1] >> 8; ds.run.bad_reason = (uint32_t)(D.h_ctr.p[1] & 0xFFu);
    ds.bad_is_record = 1;
}

// rec, off: n records that bam_sort_device has just passed and sorted (moni_ctx::bsort.idx[1]: place i takes record idx[1][i]).  Leaves the
// entries in D.h_ent and their number in ds.entries; the stream is synchronised.  A bad record: MONI_EINVAL with ds.run's three fields set.
static int bam_dup_device(moni_ctx_t* c, const uint8_t* rec, uint64_t len, const uint64_t* off, uint64_t n, uint32_t paired, moni_bam_run_dup_stats_t& ds) {
    auto& D = c->bdup;
    int rc;
    ds.entries = ds.pairs = ds.fragments = 0;
    if ((rc = D.h_ctr.ensure(8)) || (rc = D.h_ent.ensure(1))) return rc;
    if (!n) return MONI_OK;
    for (Event* e : {&D.e0, &D.e1, &D.e2, &D.e3, &D.e4})
        if (!e->h) HIPCHK(hipEventCreate(&e->h));
    const uint64_t n_units = paired ? (n + 1) / 2 : n;
    if ((rc = D.sig.ensure(n)) || (rc = D.where.ensure(n)) || (rc = D.cnt.ensure(n_units + 1)) || (rc = D.pos.ensure(n_units + 1)) || (rc = D.ent.ensure(n)) ||
        (rc = D.ctr.ensure(8)))
        return rc;
    bamdup_args_t G;
    memset(&G, 0, sizeof G);
    G.rec = rec; G.len = len; G.off = off; G.n = n; G.n_ref = c->bam.dict.n_ref; G.paired = paired; G.sig = D.sig.p; G.perm = c->bsort.idx[1].p; G.where = D.where.p;
    G.n_units = n_units; G.cnt = D.cnt.p; G.pos = D.pos.p; G.ent = D.ent.p; G.ctr = D.ctr.p;
    const dim3 lanes((unsigned)((n + BAMSORT_T - 1) / BAMSORT_T)), units((unsigned)((n_units + 1 + BAMSORT_T - 1) / BAMSORT_T));
    HIPCHK(hipMemsetAsync(D.ctr.p, 0, sizeof(unsigned long long), c->stream));
    HIPCHK(hipMemsetAsync(D.ctr.p + 1, 0xFF, sizeof(unsigned long long), c->stream));
    HIPCHK(hipEventRecord(D.e0, c->stream));
    hipLaunchKernelGGL(bam_dupsig_kernel, dim3((unsigned)std::min<uint64_t>((n + BAMSORT_T / BAM_W - 1) / (BAMSORT_T / BAM_W), (uint64_t)ctx_n_cu(c) * 8)), dim3(BAMSORT_T), 0,
                       c->stream, G);
    HIPCHK(hipEventRecord(D.e1, c->stream));
    hipLaunchKernelGGL(bam_dupinv_kernel, lanes, dim3(BAMSORT_T), 0, c->stream, G);
    hipLaunchKernelGGL(bam_dupunit_kernel<false>, units, dim3(BAMSORT_T), 0, c->stream, G);
    if ((rc = exclusive_scan_u64(c, D.cnt.p, D.pos.p, n_units + 1))) return rc;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(D.h_ctr.p, D.ctr.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(D.h_ctr.p + 2, D.pos.p + n_units, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (D.h_ctr.p[0]) { bam_dup_bad(c, ds); return MONI_EINVAL; }
    const uint64_t n_ent = D.h_ctr.p[2];
    if (n_ent > n) { fprintf(stderr, "moni_hip: duplicate marking: the units' entry counts are inconsistent\n"); return MONI_ERANGE; }
    if ((rc = D.h_ent.ensure(n_ent + 1))) return rc;
    hipLaunchKernelGGL(bam_dupunit_kernel<true>, units, dim3(BAMSORT_T), 0, c->stream, G);
    HIPCHK(hipEventRecord(D.e2, c->stream));
    HIPCHK(hipGetLastError());
    if (n_ent) HIPCHK(hipMemcpyAsync(D.h_ent.p, D.ent.p, n_ent * sizeof(moni_bam_dup_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, D.e0, D.e1)); ds.t_sig = ms * 1e-3;
    HIPCHK(hipEventElapsedTime(&ms, D.e1, D.e2)); ds.t_entry = ms * 1e-3;
    ds.entries = n_ent;
    for (uint64_t j = 0; j < n_ent; ++j) ds.pairs += D.h_ent.p[j].kind != 0;
    ds.fragments = n_ent - ds.pairs;
    return MONI_OK;
}

// the marks of moni_bam_sort_marked onto the device copy of its records, before any check: the kernel stays inside rec[0, len)
static int bam_setdup_device(moni_ctx_t* c, uint8_t* rec, uint64_t len, const uint64_t* off, uint64_t n, const uint8_t* marks) {
    auto& D = c->bdup;
    int rc;
    if (!n) return MONI_OK;
    if ((rc = D.marks_in.ensure(n))) return rc;
    HIPCHK(hipMemcpyAsync(D.marks_in.p, marks, n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(bam_setdup_kernel, dim3((unsigned)((n + BAMSORT_T - 1) / BAMSORT_T)), dim3(BAMSORT_T), 0, c->stream, rec, len, off, n, D.marks_in.p);
    HIPCHK(hipGetLastError());
    return MONI_OK;
}

int moni_bam_sorted_run_dup(moni_ctx_t* c, const void* sam_lines, uint64_t len, uint32_t paired, const uint8_t** records, uint64_t* records_len, const uint64_t** keys,
                            const uint64_t** offs, uint64_t* n, const moni_bam_dup_t** dups, uint64_t* n_dups, moni_bam_run_dup_stats_t* stats) {
    if (!dups || !n_dups || paired > 1u) return MONI_EINVAL;
    moni_bam_run_dup_stats_t ds;
    memset(&ds, 0, sizeof ds);
    *n_dups = 0;
    const int rc = bam_sorted_run_core(c, sam_lines, len, records, records_len, keys, offs, n, &ds.run, paired, &ds);
    if (rc == MONI_OK) { *dups = c->bdup.h_ent.p; *n_dups = ds.entries; }
    if (stats) *stats = ds;
    return rc;
}

int moni_bam_sort_marked(moni_ctx_t* c, const void* records, uint64_t len, const uint64_t* offs, uint64_t n, const uint8_t* marks, const moni_bam_params_t* prm,
                         const uint8_t** out, uint64_t* out_len, const moni_bam_ent_t** ents, moni_bam_sort_stats_t* stats) {
    return bam_sort_core(c, records, len, offs, n, marks, prm, out, out_len, ents, stats);
}

int moni_bam_dup_resolve(moni_ctx_t* c, const moni_bam_dup_t* const* dups, const uint64_t* n_dups, const uint64_t* n_records, uint64_t n_runs, uint8_t* const* marks,
                         moni_bam_dup_stats_t* stats) {
    if (!c || (n_runs && (!dups || !n_dups || !n_records || !marks)) || !c->bam.has_header) return MONI_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    moni_bam_dup_stats_t st;
    memset(&st, 0, sizeof st);
    if (stats) *stats = st;
    uint64_t N = 0, M = 0;
    for (uint64_t r = 0; r < n_runs; ++r) {
        if ((n_dups[r] && !dups[r]) || (n_records[r] && !marks[r])) return MONI_EINVAL;
        N += n_dups[r]; M += n_records[r];
        if (N >= (1ull << 31) || M >= 0xFFFFFFFFull) return MONI_ERANGE;
    }
    HIPCHK(hipSetDevice(c->idx->device));
    auto& D = c->bdup;
    int rc = MONI_OK;
    if (N) {
        for (Event* e : {&D.e0, &D.e1, &D.e2, &D.e3, &D.e4})
            if (!e->h) HIPCHK(hipEventCreate(&e->h));
        const uint32_t ebits = bam_dup_bits(c->bam.dict.n_ref);
        size_t tmp_bytes = 0;
        if (rocprim::radix_sort_pairs(nullptr, tmp_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)(2 * N), 0u, 64u, c->stream) != hipSuccess)
            return MONI_ENODEV;
        if ((rc = D.all.ensure(N)) || (rc = D.base.ensure(2 * (n_runs + 1))) || (rc = D.pkey.ensure(N)) || (rc = D.ekey.ensure(2 * N)) || (rc = D.key[0].ensure(2 * N)) ||
            (rc = D.key[1].ensure(2 * N)) || (rc = D.at.ensure(2 * N)) || (rc = D.pidx.ensure(N)) || (rc = D.eidx.ensure(2 * N)) || (rc = D.idx[0].ensure(2 * N)) ||
            (rc = D.idx[1].ensure(2 * N)) || (rc = D.marks.ensure(M + 1)) || (rc = D.sort_tmp.ensure(tmp_bytes + 16)) || (rc = D.ctr.ensure(8)) || (rc = D.h_ctr.ensure(8)))
            return rc;
        std::vector<uint64_t> base(2 * (n_runs + 1), 0);          // where the runs' entries begin, then where their marks begin
        for (uint64_t r = 0; r < n_runs; ++r) { base[r + 1] = base[r] + n_dups[r]; base[n_runs + 2 + r] = base[n_runs + 1 + r] + n_records[r]; }
        HIPCHK(hipMemcpyAsync(D.base.p, base.data(), base.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        for (uint64_t r = 0; r < n_runs; ++r)
            if (n_dups[r]) HIPCHK(hipMemcpyAsync(D.all.p + base[r], dups[r], n_dups[r] * sizeof(moni_bam_dup_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemsetAsync(D.ctr.p, 0, 8 * sizeof(unsigned long long), c->stream));
        HIPCHK(hipMemsetAsync(D.ctr.p + 1, 0xFF, sizeof(unsigned long long), c->stream));
        HIPCHK(hipMemsetAsync(D.marks.p, 0, M + 1, c->stream));
        bamres_args_t R;
        memset(&R, 0, sizeof R);
        R.ent = D.all.p; R.n_ent = N; R.ent_base = D.base.p; R.rec_base = D.base.p + n_runs + 1; R.n_runs = n_runs; R.at = D.at.p; R.pkey = D.pkey.p; R.ekey = D.ekey.p;
        R.pidx = D.pidx.p; R.eidx = D.eidx.p; R.marks = D.marks.p; R.ctr = D.ctr.p;
        const dim3 ln((unsigned)((N + BAMSORT_T - 1) / BAMSORT_T)), ln2((unsigned)((2 * N + BAMSORT_T - 1) / BAMSORT_T));
        HIPCHK(hipEventRecord(D.e0, c->stream));
        hipLaunchKernelGGL(bam_dupprep_kernel, ln, dim3(BAMSORT_T), 0, c->stream, R);
        HIPCHK(hipEventRecord(D.e1, c->stream));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(D.h_ctr.p, D.ctr.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        st.entries = N;
        if (D.h_ctr.p[0]) {          // before any pass that trusts the places
            st.bad_entries = D.h_ctr.p[0]; st.first_bad_entry = D.h_ctr.p[1];
            st.t_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (stats) *stats = st;
            return MONI_EINVAL;
        }
        auto sort = [&](uint64_t* ki, uint64_t* ko, uint32_t* vi, uint32_t* vo, uint64_t n, uint32_t bits) {
            return rocprim::radix_sort_pairs(D.sort_tmp.p, tmp_bytes, ki, ko, vi, vo, (size_t)n, 0u, bits, c->stream) == hipSuccess;
        };
        auto keys = [&](const uint32_t* perm, uint32_t pass) {
            R.perm = perm; R.key = D.key[0].p; R.pass = pass;
            hipLaunchKernelGGL(bam_dupkey_kernel, pass == 3u ? ln2 : ln, dim3(BAMSORT_T), 0, c->stream, R);
        };
        // the pairs: by (k1, k2, kind, score descending, ordinal), the least significant key first
        if (!sort(D.pkey.p, D.key[1].p, D.pidx.p, D.idx[1].p, N, 34u)) return MONI_ENODEV;
        keys(D.idx[1].p, 1u);
        if (!sort(D.key[0].p, D.key[1].p, D.idx[1].p, D.idx[0].p, N, ebits)) return MONI_ENODEV;
        keys(D.idx[0].p, 2u);
        if (!sort(D.key[0].p, D.key[1].p, D.idx[0].p, D.idx[1].p, N, ebits)) return MONI_ENODEV;
        HIPCHK(hipEventRecord(D.e2, c->stream));
        R.perm = D.idx[1].p;
        hipLaunchKernelGGL(bam_duppair_kernel, ln, dim3(BAMSORT_T), 0, c->stream, R);
        HIPCHK(hipEventRecord(D.e3, c->stream));
        // the ends: by (e, class, score descending, ordinal).  The empty second slot of a fragment has every bit of e set: it may land in the last
        // group of the live bits, behind that group's fragments (its class is the last), where no flag looks at it
        if (!sort(D.ekey.p, D.key[1].p, D.eidx.p, D.idx[1].p, 2 * N, 34u)) return MONI_ENODEV;
        keys(D.idx[1].p, 3u);
        if (!sort(D.key[0].p, D.key[1].p, D.idx[1].p, D.idx[0].p, 2 * N, ebits)) return MONI_ENODEV;
        HIPCHK(hipEventRecord(D.e4, c->stream));
        R.perm = D.idx[0].p;
        hipLaunchKernelGGL(bam_dupend_kernel, ln2, dim3(BAMSORT_T), 0, c->stream, R);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(D.h_ctr.p, D.ctr.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        for (uint64_t r = 0; r < n_runs; ++r)
            if (n_records[r]) HIPCHK(hipMemcpyAsync(marks[r], D.marks.p + base[n_runs + 1 + r], n_records[r], hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        float a = 0, b = 0;
        HIPCHK(hipEventElapsedTime(&a, D.e1, D.e2)); HIPCHK(hipEventElapsedTime(&b, D.e3, D.e4)); st.t_sort = (a + b) * 1e-3;          // with the key kernels between the passes
        HIPCHK(hipEventElapsedTime(&a, D.e0, D.e1)); HIPCHK(hipEventElapsedTime(&b, D.e2, D.e3)); st.t_flag = (a + b) * 1e-3;          // the end flags run behind the last event
        st.pairs = D.h_ctr.p[2]; st.dup_pairs = D.h_ctr.p[3]; st.fragments = D.h_ctr.p[4]; st.dup_fragments = D.h_ctr.p[5];
        st.marked_records = 2 * st.dup_pairs + st.dup_fragments;
    } else {
        for (uint64_t r = 0; r < n_runs; ++r)
            if (n_records[r]) memset(marks[r], 0, n_records[r]);
    }
    st.t_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = st;
    return rc;
}
