// Host side of the BAM reader (included inside extern "C" of moni_hip.hip): the kernels are in bamin_kernels.hip, DESIGN.md 7.16 has the plan.
// One feed = the call's members inflated directly behind the carry (infl_table / infl_launch of inflate_api.inc, with this feature's own
// tables), then per group of BAMIN_GROUP segments sweep, chain and list - launches in stream order, no host in between -, a scan of the
// segments' counts and the compaction; then the selection with rocPRIM's scans, the text, and the new carry.  The host waits four times:
// for the members' statuses, for the record count, for the text lengths, for the text.  Nothing of the stream's state (carry, header,
// record count) changes before the call is known to be good.  All buffers are moni_ctx::bamin's own, grow-only.

void moni_bamin_params_default(moni_bamin_params_t* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->check_crc = 1;
}

int moni_bam_in_reset(moni_ctx_t* c) {
    if (!c) return MONI_EINVAL;
    c->bamin.carry_len = 0; c->bamin.rec_base = 0; c->bamin.header_done = false;
    return MONI_OK;
}

int moni_bam_in_feed(moni_ctx_t* c, const void* blocks, uint64_t len, const moni_bamin_params_t* prm, int last, const uint8_t** text1, uint64_t* len1,
                     const uint8_t** text2, uint64_t* len2, uint64_t* n_reads, moni_bamin_stats_t* stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (!c || !prm || !text1 || !len1 || !text2 || !len2 || !n_reads || prm->paired > 1 || prm->check_crc > 1 || prm->reserved[0] || prm->reserved[1] ||
        last < 0 || last > 1 || (!blocks && len))
        return MONI_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    auto& B = c->bamin;
    const uint8_t* d = static_cast<const uint8_t*>(blocks);
    moni_bamin_stats_t st;
    memset(&st, 0, sizeof st);
    st.inflate.in_bytes = len; st.carried_bytes = B.carry_len; st.header_done = B.header_done ? 1u : 0u;
    *text1 = nullptr; *text2 = nullptr; *len1 = *len2 = *n_reads = 0;
    auto done = [&](int rc) {
        st.t_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = st;
        return rc;
    };
    if (!len && !last) return done(MONI_OK);
    HIPCHK(hipSetDevice(c->idx->device));
    for (Event& e : B.e)
        if (!e.h) HIPCHK(hipEventCreate(&e.h));
    int rc, scan = MONI_OK;

    // ---- the stream: the carry, the members' text directly behind it
    uint64_t nb = 0, used = 0, text = 0;
    if (len && (rc = infl_table(B.inf, d, len, nb, used, text, scan))) return rc;
    const uint64_t carry = B.carry_len, N = carry + text;
    if (N >> 32) return MONI_ERANGE;
    if ((rc = B.stream.ensure(N + 16)) || (rc = B.st.ensure(1)) || (rc = B.h_st.ensure(1)) || (rc = B.h_sum.ensure(1))) return rc;
    if (carry) HIPCHK(hipMemcpyAsync(B.stream.p, B.carry.p, carry, hipMemcpyDeviceToDevice, c->stream));
    if (nb) {
        if ((rc = infl_launch(c, B.inf, d, used, nb, B.stream.p + carry, prm->check_crc))) return rc;
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if ((rc = infl_verdict(B.inf, nb, text, used < len, scan == MONI_EINVAL ? MONI_INF_HEADER : MONI_INF_TRUNCATED, st.inflate))) return rc;
    st.t_kernel[0] = st.inflate.t_kernel;
    if (st.inflate.bad_blocks) return done(MONI_EINVAL);

    bamin_state_t& H = *B.h_st.p;
    memset(&H, 0, sizeof H);
    H.pending = B.header_done ? 0ull : BAMIN_END; H.carry_off = N; H.bad = ~0ull; H.rec_base = B.rec_base; H.lone_rec = ~0ull; H.header_done = B.header_done ? 1u : 0u;
    uint64_t n_rec = 0;
    bamin_args_t G;
    memset(&G, 0, sizeof G);
    if (N) {
        // ---- where the records start
        const uint64_t n_seg = (N + BAMIN_S - 1u) / BAMIN_S, group = std::min<uint64_t>(n_seg, BAMIN_GROUP);
        if ((rc = B.table.ensure(group * BAMIN_S)) || (rc = B.entry.ensure(n_seg)) || (rc = B.slots.ensure(n_seg * BAMIN_SLOTS)) || (rc = B.cnt.ensure(n_seg + 1)) ||
            (rc = B.pos.ensure(n_seg + 1)) || (rc = B.seg_bad.ensure(n_seg)) || (rc = B.rec_off.ensure(N / BAM_FIXED + 2)))
            return rc;
        G.s = B.stream.p; G.n = N; G.st = B.st.p; G.table = B.table.p; G.entry = B.entry.p; G.n_seg = n_seg; G.slots = B.slots.p; G.cnt = B.cnt.p;
        G.seg_bad = B.seg_bad.p; G.pos = B.pos.p; G.rec_off = B.rec_off.p; G.paired = prm->paired;
        HIPCHK(hipMemcpyAsync(B.st.p, &H, sizeof H, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipEventRecord(B.e[0], c->stream));
        for (uint64_t k0 = 0; k0 < n_seg; k0 += BAMIN_GROUP) {
            G.k0 = k0; G.k1 = std::min<uint64_t>(n_seg, k0 + BAMIN_GROUP);
            const unsigned segs = (unsigned)(G.k1 - G.k0);
            hipLaunchKernelGGL(bamin_sweep_kernel, dim3(std::min<unsigned>(segs, (unsigned)ctx_n_cu(c) * 2u)), dim3(BAMIN_T), 0, c->stream, G);          // 64 KB of LDS each: two to a CU
            hipLaunchKernelGGL(bamin_chain_kernel, dim3(1), dim3(64), 0, c->stream, G);
            hipLaunchKernelGGL(bamin_list_kernel, dim3((segs + BAMIN_T - 1u) / BAMIN_T), dim3(BAMIN_T), 0, c->stream, G);
        }
        HIPCHK(hipGetLastError());
        if ((rc = exclusive_scan_u64(c, B.cnt.p, B.pos.p, n_seg + 1))) return rc;
        hipLaunchKernelGGL(bamin_compact_kernel, dim3((unsigned)n_seg), dim3(BAMIN_T), 0, c->stream, G);
        HIPCHK(hipEventRecord(B.e[1], c->stream));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(B.h_sum.p, B.pos.p + n_seg, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(&H, B.st.p, sizeof H, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        n_rec = *B.h_sum.p;
    }
    if (n_rec) {
        // ---- which records give a read, and where its text goes
        if ((rc = B.cls.ensure(n_rec + 1)) || (rc = B.cls_x.ensure(n_rec + 1)) || (rc = B.len1.ensure(n_rec + 1)) || (rc = B.len1_x.ensure(n_rec + 1))) return rc;
        if (prm->paired && ((rc = B.len2.ensure(n_rec + 1)) || (rc = B.len2_x.ensure(n_rec + 1)) || (rc = B.kept_off.ensure(n_rec + 1)))) return rc;
        G.n_rec = n_rec; G.cls = B.cls.p; G.cls_x = B.cls_x.p; G.len1 = B.len1.p; G.len2 = B.len2.p; G.len1_x = B.len1_x.p; G.len2_x = B.len2_x.p; G.kept_off = B.kept_off.p;
        const unsigned rgrid = (unsigned)((n_rec + 1 + BAMIN_T - 1u) / BAMIN_T);
        HIPCHK(hipEventRecord(B.e[2], c->stream));
        hipLaunchKernelGGL(bamin_select_kernel, dim3(rgrid), dim3(BAMIN_T), 0, c->stream, G);
        if ((rc = exclusive_scan_u64(c, B.cls.p, B.cls_x.p, n_rec + 1))) return rc;
        if (prm->paired) hipLaunchKernelGGL(bamin_rank_kernel, dim3(rgrid), dim3(BAMIN_T), 0, c->stream, G);
        if ((rc = exclusive_scan_u64(c, B.len1.p, B.len1_x.p, n_rec + 1))) return rc;
        if (prm->paired && (rc = exclusive_scan_u64(c, B.len2.p, B.len2_x.p, n_rec + 1))) return rc;
        hipLaunchKernelGGL(bamin_summary_kernel, dim3(1), dim3(64), 0, c->stream, G);
        HIPCHK(hipEventRecord(B.e[3], c->stream));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&H, B.st.p, sizeof H, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        // ---- the text
        if ((rc = B.text1.ensure(H.len1 + 1)) || (rc = B.h_text1.ensure(H.len1 + 1)) || (rc = B.text2.ensure(H.len2 + 1)) || (rc = B.h_text2.ensure(H.len2 + 1))) return rc;
        G.text1 = B.text1.p; G.text2 = B.text2.p;
        if (H.len1 + H.len2) {
            HIPCHK(hipEventRecord(B.e[4], c->stream));
            hipLaunchKernelGGL(bamin_fastq_kernel, dim3((unsigned)std::min<uint64_t>((n_rec + 3) / 4, (uint64_t)ctx_n_cu(c) * 16)), dim3(BAMIN_T), 0, c->stream, G);
            HIPCHK(hipEventRecord(B.e[5], c->stream));
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(&H.bad, &B.st.p->bad, sizeof H.bad, hipMemcpyDeviceToHost, c->stream));
            if (H.len1) HIPCHK(hipMemcpyAsync(B.h_text1.p, B.text1.p, H.len1, hipMemcpyDeviceToHost, c->stream));
            if (H.len2) HIPCHK(hipMemcpyAsync(B.h_text2.p, B.text2.p, H.len2, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
    }
    float ms = 0;
    if (N) { HIPCHK(hipEventElapsedTime(&ms, B.e[0], B.e[1])); st.t_kernel[1] = ms * 1e-3; }
    if (n_rec) { HIPCHK(hipEventElapsedTime(&ms, B.e[2], B.e[3])); st.t_kernel[2] = ms * 1e-3; }
    if (n_rec && H.len1 + H.len2) { HIPCHK(hipEventElapsedTime(&ms, B.e[4], B.e[5])); st.t_kernel[3] = ms * 1e-3; }

    // ---- the verdict; only a good call moves the stream on
    const uint64_t left = N - H.carry_off;
    if (H.bad == ~0ull && last && left) H.bad = (B.rec_base + H.seen) << 8 | MONI_BAMIN_TRUNCATED;
    if (H.bad != ~0ull) {
        st.bad_records = 1; st.first_bad_record = H.bad >> 8; st.bad_record_reason = (uint32_t)(H.bad & 255u);
        return done(MONI_EINVAL);
    }
    if (left) {
        if ((rc = B.carry.ensure(left))) return rc;
        HIPCHK(hipMemcpyAsync(B.carry.p, B.stream.p + H.carry_off, left, hipMemcpyDeviceToDevice, c->stream));
    }
    B.carry_len = left; B.rec_base += H.seen; B.header_done = H.header_done != 0u;
    st.records = H.seen; st.reads = H.kept; st.skipped_secondary = H.skipped_sec; st.skipped_empty = H.skipped_empty;
    st.carried_bytes = left; st.header_done = H.header_done;
    *text1 = B.h_text1.p; *len1 = H.len1; *n_reads = prm->paired ? H.kept / 2u : H.kept;
    if (prm->paired) { *text2 = B.h_text2.p; *len2 = H.len2; }
    return done(MONI_OK);
}
