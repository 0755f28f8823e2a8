// Host side of the BAM encoder (included inside extern "C" of moni_hip.hip, behind bgzf_api.inc): the kernels are in bam_kernels.hip.
// One call = the text to the device, the two newline passes around a scan (where every line begins), the size pass (bam_line<false>: the
// records' sizes, the bad lines), a scan of the sizes, the write pass (bam_line<true>); then the records, still on the device, go through
// bgzf_compress_device - or, with raw, to the pinned buffer as they are.  All buffers are the context's own (moni_ctx::bam and, for the
// blocks, moni_ctx::bz): the resident batch and every earlier result stay as they are.

void moni_bam_params_default(moni_bam_params_t* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->block_size = BGZF_MAX_BLOCK; p->level = 1;
}

int moni_bam_set_header(moni_ctx_t* c, const char* sam_header, uint64_t len, const uint8_t** bam_header, uint64_t* bam_header_len) {
    if (!c || (!sam_header && len) || !bam_header || !bam_header_len) return MONI_EINVAL;
    bam_header_t H;
    if (!bam_header_build(sam_header ? sam_header : "", len, H)) return MONI_EINVAL;
    HIPCHK(hipSetDevice(c->idx->device));
    auto& B = c->bam;
    int rc;
    if ((rc = B.names.ensure(H.names.size() + 1)) || (rc = B.refs.ensure(H.refs.size() + 1)) || (rc = B.slots.ensure(H.slots.size()))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));          // nothing of an earlier call reads the old dictionary any more
    if (!H.names.empty()) HIPCHK(hipMemcpy(B.names.p, H.names.data(), H.names.size(), hipMemcpyHostToDevice));
    if (!H.refs.empty()) HIPCHK(hipMemcpy(B.refs.p, H.refs.data(), H.refs.size() * sizeof(bam_ref_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(B.slots.p, H.slots.data(), H.slots.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    B.dict.names = B.names.p; B.dict.refs = B.refs.p; B.dict.slots = B.slots.p;
    B.dict.mask = (uint32_t)H.slots.size() - 1u; B.dict.n_ref = (uint32_t)H.refs.size();
    B.header.swap(H.bam);
    B.has_header = true;
    *bam_header = B.header.data(); *bam_header_len = B.header.size();
    return MONI_OK;
}

// The encoder's passes over `len` bytes of SAM lines: *n_lines records of *total bytes in all stay on the device, in B.out at the offsets B.off
// (n_lines + 1 entries); the write pass is launched, not waited for.  st: in_bytes, lines, the bad lines; t_encode is the caller's to read from
// B.e0 / B.e1 once the stream has been synchronised.  MONI_EINVAL with st.bad_lines set: a bad line, nothing was written.
static int bam_encode_device(moni_ctx_t* c, const void* sam_lines, uint64_t len, uint64_t* n_lines_out, uint64_t* total_out, moni_bam_stats_t& st) {
    HIPCHK(hipSetDevice(c->idx->device));
    auto& B = c->bam;
    const uint8_t* text = static_cast<const uint8_t*>(sam_lines);
    memset(&st, 0, sizeof st);
    st.in_bytes = len;
    *n_lines_out = 0; *total_out = 0;
    int rc;
    if ((rc = B.h_sum.ensure(8)) || (rc = B.ctr.ensure(2)) || (rc = B.h_out.ensure(1))) return rc;
    if (len && text[len - 1] != '\n') {          // the one check that needs no parse: the index of the unterminated line is the number of \n before it
        for (const uint8_t* p = text; (p = static_cast<const uint8_t*>(memchr(p, '\n', (size_t)(text + len - p)))) != nullptr; ++p) ++st.first_bad_line;
        st.bad_lines = 1; st.bad_reason = MONI_BAM_NEWLINE;
        return MONI_EINVAL;
    }
    uint64_t total = 0;
    if (len) {
        const uint64_t n_tiles = (len + BAM_TILE - 1) / BAM_TILE;
        auto grid = [&](uint64_t waves) { return dim3((unsigned)std::min<uint64_t>((waves + BAM_T / BAM_W - 1) / (BAM_T / BAM_W), (uint64_t)ctx_n_cu(c) * 8)); };
        if ((rc = B.text.ensure(len)) || (rc = B.tile_cnt.ensure(n_tiles + 1)) || (rc = B.tile_pos.ensure(n_tiles + 1))) return rc;
        if (!B.e0.h) HIPCHK(hipEventCreate(&B.e0.h));
        if (!B.e1.h) HIPCHK(hipEventCreate(&B.e1.h));
        bam_args_t G;
        memset(&G, 0, sizeof G);
        G.text = B.text.p; G.len = len; G.n_tiles = n_tiles; G.tile_cnt = B.tile_cnt.p; G.tile_pos = B.tile_pos.p; G.ctr = B.ctr.p; G.dict = B.dict;
        HIPCHK(hipMemcpyAsync(B.text.p, text, len, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemsetAsync(B.tile_cnt.p + n_tiles, 0, sizeof(uint64_t), c->stream));          // the scan's last entry: the sum
        HIPCHK(hipMemsetAsync(B.ctr.p, 0, sizeof(unsigned long long), c->stream));
        HIPCHK(hipMemsetAsync(B.ctr.p + 1, 0xFF, sizeof(unsigned long long), c->stream));
        HIPCHK(hipEventRecord(B.e0, c->stream));
        hipLaunchKernelGGL(bam_count_kernel, grid(n_tiles), dim3(BAM_T), 0, c->stream, G);
        if ((rc = exclusive_scan_u64(c, B.tile_cnt.p, B.tile_pos.p, n_tiles + 1))) return rc;
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(B.h_sum.p, B.tile_pos.p + n_tiles, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        const uint64_t n_lines = B.h_sum.p[0];          // at least one: the text ends in \n
        if (!n_lines || n_lines > len) { fprintf(stderr, "moni_hip: bam: the line count is inconsistent\n"); return MONI_ERANGE; }
        if ((rc = B.starts.ensure(n_lines + 1)) || (rc = B.size.ensure(n_lines + 1)) || (rc = B.off.ensure(n_lines + 1))) return rc;
        G.n_lines = n_lines; G.starts = B.starts.p; G.size = B.size.p; G.off = B.off.p;
        HIPCHK(hipMemsetAsync(B.starts.p, 0, sizeof(uint64_t), c->stream));          // line 0 begins at 0
        HIPCHK(hipMemsetAsync(B.size.p + n_lines, 0, sizeof(uint64_t), c->stream));
        hipLaunchKernelGGL(bam_starts_kernel, grid(n_tiles), dim3(BAM_T), 0, c->stream, G);
        hipLaunchKernelGGL(bam_size_kernel, grid(n_lines), dim3(BAM_T), 0, c->stream, G);
        if ((rc = exclusive_scan_u64(c, B.size.p, B.off.p, n_lines + 1))) return rc;
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(B.h_sum.p, B.off.p + n_lines, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(B.h_sum.p + 1, B.ctr.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        st.lines = n_lines;
        if (B.h_sum.p[1]) {
            st.bad_lines = B.h_sum.p[1]; st.first_bad_line = B.h_sum.p[2] >> 8; st.bad_reason = (uint32_t)(B.h_sum.p[2] & 0xFFu);
            return MONI_EINVAL;
        }
        total = B.h_sum.p[0];
        // a record is at most 36 + its line's bytes + 3 per tag field more than the text spent on it: far inside 2 * len + 36 * lines
        if (total > 2 * len + (uint64_t)BAM_FIXED * n_lines) { fprintf(stderr, "moni_hip: bam: the records' sizes are inconsistent\n"); return MONI_ERANGE; }
        if ((rc = B.out.ensure(total + 8))) return rc;
        G.out = B.out.p;
        hipLaunchKernelGGL(bam_write_kernel, grid(n_lines), dim3(BAM_T), 0, c->stream, G);
        HIPCHK(hipEventRecord(B.e1, c->stream));
        HIPCHK(hipGetLastError());
        *n_lines_out = st.lines;
    }
    st.bam_bytes = total;
    *total_out = total;
    return MONI_OK;
}

int moni_bam_records(moni_ctx_t* c, const void* sam_lines, uint64_t len, const moni_bam_params_t* prm, const uint8_t** out, uint64_t* out_len,
                     moni_bam_stats_t* stats) {
    if (!c || !prm || !out || !out_len || (!sam_lines && len)) return MONI_EINVAL;
    const moni_bgzf_params_t zp = {prm->block_size, prm->level, prm->raw ? 0u : prm->eof, 0u};
    if (!bgzf_params_ok(zp) || prm->eof > 1u || prm->raw > 1u || prm->reserved[0] || prm->reserved[1] || !c->bam.has_header) return MONI_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    auto& B = c->bam;
    moni_bam_stats_t st;
    *out_len = 0;
    uint64_t n_lines = 0, total = 0;
    int rc = bam_encode_device(c, sam_lines, len, &n_lines, &total, st);
    if (rc) {
        if (rc == MONI_EINVAL && st.bad_lines) {
            st.t_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (stats) *stats = st;
        }
        return rc;
    }
    if (prm->raw) {
        if ((rc = B.h_out.ensure(total + 1))) return rc;
        if (total) HIPCHK(hipMemcpyAsync(B.h_out.p, B.out.p, total, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        *out = B.h_out.p; *out_len = total;
        st.out_bytes = total;
    } else {
        moni_bgzf_stats_t zs;
        if ((rc = bgzf_compress_device(c, B.out.p, total, &zp, out, out_len, zs))) return rc;
        st.out_bytes = zs.out_bytes; st.blocks = zs.blocks; st.t_deflate = zs.t_kernel;
    }
    if (len) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, B.e0, B.e1));
        st.t_encode = ms * 1e-3;
    }
    st.t_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = st;
    return MONI_OK;
}
