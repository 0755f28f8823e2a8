// Host side of the BGZF reader (included inside extern "C" of moni_hip.hip): the kernel is in inflate_kernels.hip.
// One call = a walk over the members' headers on the host (where each starts, where its text goes), the members and that table to the
// device, inflate_member_kernel (a wavefront per member into the member's slot of the text), one transfer into the context's pinned
// buffer.  All buffers are the context's own (moni_ctx::inf): the resident batch and every earlier result stay as they are.

void moni_inflate_params_default(moni_inflate_params_t* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->check_crc = 1;
}

int moni_bgzf_scan(const void* data, uint64_t len, uint64_t* n_blocks, uint64_t* used, uint64_t* out_bytes) {
    if (!data && len) return MONI_EINVAL;
    const uint8_t* d = static_cast<const uint8_t*>(data);
    uint64_t at = 0, nb = 0, ob = 0;
    int rc = 0;
    infl_member_t m;
    while (at < len && (rc = infl_member_at(d, len, at, m)) == 0) { at += m.pay_off + m.pay_len + 8u; nb += 1; ob += m.isize; }
    if (n_blocks) *n_blocks = nb;
    if (used) *used = at;
    if (out_bytes) *out_bytes = ob;
    return rc == 2 ? MONI_EINVAL : MONI_OK;
}

// The members of d[0, len): how many are whole and what they take (moni_bgzf_scan), their table in I.h_mem with the slots of the text back to
// back from 0, `text` bytes in all.
static int infl_table(moni_ctx::InflateBufs& I, const uint8_t* d, uint64_t len, uint64_t& nb, uint64_t& used, uint64_t& text, int& scan) {
    nb = used = text = 0;
    scan = moni_bgzf_scan(d, len, &nb, &used, nullptr);
    int rc;
    if ((rc = I.h_mem.ensure(nb + 1))) return rc;
    for (uint64_t b = 0, at = 0; b < nb; ++b) {
        infl_member_t& m = I.h_mem.p[b];
        infl_member_at(d, len, at, m);
        m.out_off = text;
        text += infl_slot_bytes(m.isize);
        at += m.pay_off + m.pay_len + 8u;
    }
    return MONI_OK;
}

// The nb > 0 members of infl_table and their table to the device, inflate_member_kernel over them into out (device memory, the table's `text`
// bytes) between the events e0 and e1, the statuses and the counters on their way back.  Nothing waits: the caller synchronises the stream.
static int infl_launch(moni_ctx_t* c, moni_ctx::InflateBufs& I, const uint8_t* d, uint64_t used, uint64_t nb, uint8_t* out, uint32_t check_crc) {
    int rc;
    if ((rc = I.in.ensure(used)) || (rc = I.mem.ensure(nb)) || (rc = I.status.ensure(nb)) || (rc = I.counters.ensure(4)) || (rc = I.h_status.ensure(nb)) || (rc = I.h_ctr.ensure(4)))
        return rc;
    if (!I.e0.h) HIPCHK(hipEventCreate(&I.e0.h));
    if (!I.e1.h) HIPCHK(hipEventCreate(&I.e1.h));
    HIPCHK(hipMemcpyAsync(I.in.p, d, used, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(I.mem.p, I.h_mem.p, nb * sizeof(infl_member_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(I.counters.p, 0, 4 * sizeof(unsigned long long), c->stream));
    infl_args_t G;
    G.in = I.in.p; G.mem = I.mem.p; G.n_members = nb; G.out = out; G.status = I.status.p; G.counters = I.counters.p; G.check_crc = check_crc;
    const unsigned grid = (unsigned)std::min<uint64_t>(nb, (uint64_t)ctx_n_cu(c) * 16);          // 6 KB of LDS and a wave each: sixteen members share a CU
    HIPCHK(hipEventRecord(I.e0, c->stream));
    hipLaunchKernelGGL(inflate_member_kernel, dim3(grid), dim3(INFL_T), 0, c->stream, G);
    HIPCHK(hipEventRecord(I.e1, c->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(I.h_status.p, I.status.p, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(I.h_ctr.p, I.counters.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    return MONI_OK;
}

// Behind the stream's synchronisation: the kernel's time, the blocks by BTYPE, the bad members (tail_bad: bytes behind the last whole member)
static int infl_verdict(moni_ctx::InflateBufs& I, uint64_t nb, uint64_t text, bool tail_bad, uint32_t tail_reason, moni_inflate_stats_t& st) {
    uint64_t bad = 0, first_bad = 0;
    uint32_t reason = MONI_INF_OK;
    st.blocks = nb + (tail_bad ? 1 : 0);
    if (nb) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, I.e0, I.e1));
        st.t_kernel = ms * 1e-3;
        st.stored = I.h_ctr.p[0]; st.fixed = I.h_ctr.p[1]; st.dynamic = I.h_ctr.p[2];
        for (uint64_t b = nb; b-- > 0;)
            if (I.h_status.p[b] != MONI_INF_OK) { bad += 1; first_bad = b; reason = I.h_status.p[b]; }
    }
    if (tail_bad) {
        if (!bad) { first_bad = nb; reason = tail_reason; }
        bad += 1;
    }
    st.bad_blocks = bad; st.first_bad_block = first_bad; st.bad_reason = reason;
    st.out_bytes = bad ? 0 : text;
    return MONI_OK;
}

int moni_bgzf_inflate(moni_ctx_t* c, const void* blocks, uint64_t len, const moni_inflate_params_t* prm, const uint8_t** out, uint64_t* out_len,
                      moni_inflate_stats_t* stats) {
    if (!c || !prm || !out || !out_len || prm->check_crc > 1 || prm->reserved[0] || prm->reserved[1] || prm->reserved[2] || (!blocks && len)) return MONI_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    auto& I = c->inf;
    const uint8_t* d = static_cast<const uint8_t*>(blocks);
    moni_inflate_stats_t st;
    memset(&st, 0, sizeof st);
    st.in_bytes = len;
    *out = I.h_out.p; *out_len = 0;
    if (!len) { if (stats) *stats = st; return MONI_OK; }
    HIPCHK(hipSetDevice(c->idx->device));

    // the members: a count first (the table only grows), then the table.  A member that is no BGZF, or not whole, is bad with a reason
    // of its own; the members before it are still inflated, since the lowest bad index is what the caller is told.
    uint64_t nb = 0, used = 0, text = 0;
    int scan, rc;
    if ((rc = infl_table(I, d, len, nb, used, text, scan))) return rc;
    if (nb) {
        if ((rc = I.out.ensure(text + 1)) || (rc = I.h_out.ensure(text + 1))) return rc;
        *out = I.h_out.p;
        if ((rc = infl_launch(c, I, d, used, nb, I.out.p, prm->check_crc))) return rc;
        if (text) HIPCHK(hipMemcpyAsync(I.h_out.p, I.out.p, text, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if ((rc = infl_verdict(I, nb, text, used < len, scan == MONI_EINVAL ? MONI_INF_HEADER : MONI_INF_TRUNCATED, st))) return rc;
    st.t_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = st;
    if (st.bad_blocks) return MONI_EINVAL;
    *out_len = text;
    return MONI_OK;
}
