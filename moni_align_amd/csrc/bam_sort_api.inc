// Host side of the coordinate sort of BAM records (included inside extern "C" of moni_hip.hip, behind bam_api.inc): the kernels are in
// bam_sort_kernels.hip, the merge plan and the .bai builder in bam_index.hpp.
// One sort = bam_reckey_kernel (checks, keys, the index entries' fields), rocPRIM's radix sort of (key, record index) over the key's live bits,
// bam_place_kernel and a scan (where every record lands), bam_gather_kernel (the records and their index entries in order).  All buffers are
// the context's own (moni_ctx::bsort), grow-only: the resident batch and every earlier result stay as they are.

// rec[0, len) and off[0, n] are on the device, rec in a buffer with 8 bytes to spare behind len.  Leaves the records in B.out, their offsets
// in B.out_off, their keys in B.key[1] and their entries in B.ents, all in sorted order, and *total bytes; the stream is synchronised.
// A bad record: MONI_EINVAL with st's three fields set, and nothing gathered.
static int bam_sort_device(moni_ctx_t* c, const uint8_t* rec, uint64_t len, const uint64_t* off, uint64_t n, uint64_t* total, moni_bam_sort_stats_t& st) {
    auto& B = c->bsort;
    *total = 0;
    int rc;
    if ((rc = B.h_sum.ensure(4))) return rc;
    if (!n) return MONI_OK;
    if (n >= (1ull << 32)) return MONI_EINVAL;
    for (Event* e : {&B.e0, &B.e1, &B.e2, &B.e3, &B.e4})
        if (!e->h) HIPCHK(hipEventCreate(&e->h));
    const uint32_t n_ref = c->bam.dict.n_ref, bits = bam_key_bits(n_ref);
    size_t tmp_bytes = 0;
    if (rocprim::radix_sort_pairs(nullptr, tmp_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, 0u, bits, c->stream) != hipSuccess)
        return MONI_ENODEV;
    if ((rc = B.key[0].ensure(n)) || (rc = B.key[1].ensure(n)) || (rc = B.idx[0].ensure(n)) || (rc = B.idx[1].ensure(n)) || (rc = B.pre.ensure(n)) ||
        (rc = B.size.ensure(n + 1)) || (rc = B.out_off.ensure(n + 1)) || (rc = B.ents.ensure(n)) || (rc = B.ctr.ensure(2)) || (rc = B.sort_tmp.ensure(tmp_bytes + 16)))
        return rc;
    bamsort_args_t G;
    memset(&G, 0, sizeof G);
    G.rec = rec; G.len = len; G.off = off; G.n = n; G.n_ref = n_ref; G.key = B.key[0].p; G.idx = B.idx[0].p; G.pre = B.pre.p; G.perm = B.idx[1].p;
    G.size = B.size.p; G.out_off = B.out_off.p; G.ctr = B.ctr.p; G.ents = B.ents.p;
    const dim3 lanes((unsigned)((n + 1 + BAMSORT_T - 1) / BAMSORT_T));
    HIPCHK(hipMemsetAsync(B.ctr.p, 0, sizeof(unsigned long long), c->stream));
    HIPCHK(hipMemsetAsync(B.ctr.p + 1, 0xFF, sizeof(unsigned long long), c->stream));
    HIPCHK(hipEventRecord(B.e0, c->stream));
    hipLaunchKernelGGL(bam_reckey_kernel, lanes, dim3(BAMSORT_T), 0, c->stream, G);
    HIPCHK(hipEventRecord(B.e1, c->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(B.h_sum.p, B.ctr.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (B.h_sum.p[0]) {          // before any pass that trusts the records
        st.bad_records = B.h_sum.p[0]; st.first_bad_record = B.h_sum.p[1] >> 8; st.bad_reason = (uint32_t)(B.h_sum.p[1] & 0xFFu);
        return MONI_EINVAL;
    }
    HIPCHK(hipEventRecord(B.e2, c->stream));
    if (rocprim::radix_sort_pairs(B.sort_tmp.p, tmp_bytes, B.key[0].p, B.key[1].p, B.idx[0].p, B.idx[1].p, (size_t)n, 0u, bits, c->stream) != hipSuccess) return MONI_ENODEV;
    hipLaunchKernelGGL(bam_place_kernel, lanes, dim3(BAMSORT_T), 0, c->stream, G);
    if ((rc = exclusive_scan_u64(c, B.size.p, B.out_off.p, n + 1))) return rc;
    HIPCHK(hipEventRecord(B.e3, c->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(B.h_sum.p, B.out_off.p + n, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const uint64_t sum = B.h_sum.p[0];
    if (sum > len) { fprintf(stderr, "moni_hip: bam sort: the records' sizes are inconsistent\n"); return MONI_ERANGE; }
    if ((rc = B.out.ensure(sum + 8))) return rc;
    G.out = B.out.p;
    hipLaunchKernelGGL(bam_gather_kernel, dim3((unsigned)std::min<uint64_t>((n + BAMSORT_T / BAM_W - 1) / (BAMSORT_T / BAM_W), (uint64_t)ctx_n_cu(c) * 8)), dim3(BAMSORT_T), 0,
                       c->stream, G);
    HIPCHK(hipEventRecord(B.e4, c->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, B.e0, B.e1)); st.t_key = ms * 1e-3;
    HIPCHK(hipEventElapsedTime(&ms, B.e2, B.e3)); st.t_sort = ms * 1e-3;          // the sort, the placement and its scan
    HIPCHK(hipEventElapsedTime(&ms, B.e3, B.e4)); st.t_gather = ms * 1e-3;
    *total = sum;
    return MONI_OK;
}

// duplicate marking (bam_dup_api.inc): the entries of the run that bam_sort_device has just sorted, and the marks of moni_bam_sort_marked
static int bam_dup_device(moni_ctx_t* c, const uint8_t* rec, uint64_t len, const uint64_t* off, uint64_t n, uint32_t paired, moni_bam_run_dup_stats_t& ds);
static int bam_setdup_device(moni_ctx_t* c, uint8_t* rec, uint64_t len, const uint64_t* off, uint64_t n, const uint8_t* marks);

// moni_bam_sorted_run; with ds, moni_bam_sorted_run_dup: the entries stay in moni_ctx::bdup.h_ent, ds->entries of them
static int bam_sorted_run_core(moni_ctx_t* c, const void* sam_lines, uint64_t len, const uint8_t** records, uint64_t* records_len, const uint64_t** keys,
                               const uint64_t** offs, uint64_t* n, moni_bam_sort_stats_t* stats, uint32_t paired, moni_bam_run_dup_stats_t* ds) {
    if (!c || !records || !records_len || !keys || !offs || !n || (!sam_lines && len) || !c->bam.has_header) return MONI_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    auto& B = c->bsort;
    moni_bam_sort_stats_t st;
    memset(&st, 0, sizeof st);
    *records_len = 0; *n = 0;
    B.have_sorted = false;
    // the encoder's passes, as moni_bam_records runs them: the records stay in moni_ctx::bam.out, their offsets in moni_ctx::bam.off
    moni_bam_stats_t es;
    uint64_t n_rec = 0, enc_bytes = 0;
    int rc = bam_encode_device(c, sam_lines, len, &n_rec, &enc_bytes, es);
    st.in_bytes = len; st.records = es.lines;
    if (rc) {
        st.bad_records = es.bad_lines; st.first_bad_record = es.first_bad_line; st.bad_reason = es.bad_reason;
        st.t_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = st;
        return rc;
    }
    uint64_t total = 0;
    rc = bam_sort_device(c, c->bam.out.p, enc_bytes, c->bam.off.p, n_rec, &total, st);
    if (rc == MONI_OK && len) {          // the stream has been synchronised: the encoder's events are complete
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, c->bam.e0, c->bam.e1));
        st.t_encode = ms * 1e-3;
    }
    if (rc == MONI_OK && ds) {          // a bad record here: its figures, and nothing goes back
        rc = bam_dup_device(c, c->bam.out.p, enc_bytes, c->bam.off.p, n_rec, paired, *ds);
        if (rc == MONI_EINVAL && ds->run.bad_records) { st.bad_records = ds->run.bad_records; st.first_bad_record = ds->run.first_bad_record; st.bad_reason = ds->run.bad_reason; }
    }
    if (rc == MONI_OK) rc = B.h_rec.ensure(total + 1);
    if (rc == MONI_OK) rc = B.h_key.ensure(n_rec + 1);
    if (rc == MONI_OK) rc = B.h_off.ensure(n_rec + 1);
    if (rc == MONI_OK) {
        if (n_rec) {
            HIPCHK(hipMemcpyAsync(B.h_rec.p, B.out.p, total, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpyAsync(B.h_key.p, B.key[1].p, n_rec * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpyAsync(B.h_off.p, B.out_off.p, (n_rec + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        } else B.h_off.p[0] = 0;
        *records = B.h_rec.p; *records_len = total; *keys = B.h_key.p; *offs = B.h_off.p; *n = n_rec;
        st.bam_bytes = total; st.out_bytes = total;
        B.have_sorted = true; B.sorted_n = n_rec; B.sorted_len = total;
    }
    st.t_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = st;
    return rc;
}

int moni_bam_sorted_run(moni_ctx_t* c, const void* sam_lines, uint64_t len, const uint8_t** records, uint64_t* records_len, const uint64_t** keys,
                        const uint64_t** offs, uint64_t* n, moni_bam_sort_stats_t* stats) {
    return bam_sorted_run_core(c, sam_lines, len, records, records_len, keys, offs, n, stats, 0u, nullptr);
}

// moni_bam_sort; with marks, moni_bam_sort_marked
static int bam_sort_core(moni_ctx_t* c, const void* records, uint64_t len, const uint64_t* offs, uint64_t n, const uint8_t* marks, const moni_bam_params_t* prm,
                         const uint8_t** out, uint64_t* out_len, const moni_bam_ent_t** ents, moni_bam_sort_stats_t* stats) {
    if (!c || !prm || !out || !out_len || !ents || (!records && len) || (!offs && n)) return MONI_EINVAL;
    const moni_bgzf_params_t zp = {prm->block_size, prm->level, prm->raw ? 0u : prm->eof, 0u};
    if (!bgzf_params_ok(zp) || prm->eof > 1u || prm->raw > 1u || prm->reserved[0] || prm->reserved[1] || !c->bam.has_header) return MONI_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(c->idx->device));
    auto& B = c->bsort;
    moni_bam_sort_stats_t st;
    memset(&st, 0, sizeof st);
    st.in_bytes = len; st.records = n;
    *out_len = 0;
    B.have_sorted = false;
    int rc = MONI_OK;
    uint64_t total = 0;
    if ((n ? offs[n] : 0) != len || n >= (1ull << 32)) { st.bad_records = 1; st.first_bad_record = n; st.bad_reason = MONI_BAMSORT_LENGTH; rc = MONI_EINVAL; }
    else if ((rc = B.in.ensure(len + 8)) == MONI_OK && (rc = B.in_off.ensure(n + 1)) == MONI_OK && (rc = B.h_ents.ensure(n + 1)) == MONI_OK && n) {
        HIPCHK(hipMemcpyAsync(B.in.p, records, len, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(B.in_off.p, offs, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        if (marks) rc = bam_setdup_device(c, B.in.p, len, B.in_off.p, n, marks);
        if (rc == MONI_OK) rc = bam_sort_device(c, B.in.p, len, B.in_off.p, n, &total, st);
    }
    if (rc == MONI_OK) {
        if (n) HIPCHK(hipMemcpyAsync(B.h_ents.p, B.ents.p, n * sizeof(moni_bam_ent_t), hipMemcpyDeviceToHost, c->stream));
        if (prm->raw) {
            if ((rc = B.h_rec.ensure(total + 1))) return rc;
            if (total) HIPCHK(hipMemcpyAsync(B.h_rec.p, B.out.p, total, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            *out = B.h_rec.p; *out_len = total;
            st.out_bytes = total;
        } else {
            moni_bgzf_stats_t zs;
            if ((rc = bgzf_compress_device(c, B.out.p, total, &zp, out, out_len, zs))) return rc;          // synchronises: the entries have landed
            st.out_bytes = zs.out_bytes; st.blocks = zs.blocks; st.t_deflate = zs.t_kernel;
        }
        *ents = B.h_ents.p;
        st.bam_bytes = total;
        B.have_sorted = true; B.sorted_n = n; B.sorted_len = total;
    }
    st.t_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = st;
    return rc;
}

int moni_bam_sort(moni_ctx_t* c, const void* records, uint64_t len, const uint64_t* offs, uint64_t n, const moni_bam_params_t* prm, const uint8_t** out,
                  uint64_t* out_len, const moni_bam_ent_t** ents, moni_bam_sort_stats_t* stats) {
    return bam_sort_core(c, records, len, offs, n, nullptr, prm, out, out_len, ents, stats);
}

// ---- host only: the merge plan and the .bai builder (bam_index.hpp) ----
int moni_bam_merge_plan(const uint64_t* const* keys, const uint64_t* n, const uint64_t* const* offs, uint64_t n_runs, uint64_t chunk_bytes,
                        moni_bam_plan_t** plan) {
    if (!plan || (n_runs && (!keys || !n || !offs))) return MONI_EINVAL;
    std::vector<uint64_t> cuts;
    const int rc = bam_merge_plan(keys, n, offs, n_runs, chunk_bytes, cuts);
    if (rc) return rc;
    moni_bam_plan_t* p = static_cast<moni_bam_plan_t*>(malloc(sizeof *p));
    uint64_t* cp = static_cast<uint64_t*>(malloc((cuts.size() + 1) * sizeof(uint64_t)));
    if (!p || !cp) { free(p); free(cp); return MONI_ENOMEM; }
    memcpy(cp, cuts.data(), cuts.size() * sizeof(uint64_t));
    p->n_runs = n_runs; p->n_chunks = n_runs ? cuts.size() / n_runs - 1 : 0; p->cuts = cp;
    *plan = p;
    return MONI_OK;
}
void moni_bam_plan_free(moni_bam_plan_t* plan) {
    if (plan) { free(plan->cuts); free(plan); }
}
moni_bai_t* moni_bai_create(uint32_t n_ref) {
    moni_bai* b = new (std::nothrow) moni_bai;
    if (b) b->refs.resize(n_ref);
    return b;
}
int moni_bai_add(moni_bai_t* b, const moni_bam_ent_t* ents, uint64_t n, uint64_t chunk_len, uint32_t block_size, const uint32_t* csizes, uint64_t n_blocks,
                 uint64_t file_off) {
    return bai_add(b, ents, n, chunk_len, block_size, csizes, n_blocks, file_off);
}
int moni_bai_finish(moni_bai_t* b, uint64_t eof_off, const uint8_t** bytes, uint64_t* len) { return bai_finish(b, eof_off, bytes, len); }
void moni_bai_destroy(moni_bai_t* b) { delete b; }
