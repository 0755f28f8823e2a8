// Host side of the BGZF writer (included inside extern "C" of moni_hip.hip): the kernel is in bgzf_kernels.hip.
// One call = the text to the device (moni_bgzf_compress; the BAM path's records are there already), bgzf_block_kernel (a workgroup per BGZF block
// into the block's zeroed staging slot), a scan of the blocks' sizes, gather_lines_kernel (the slots into one stream), one transfer into the context's pinned buffer.  All buffers are the context's
// own (moni_ctx::bz): the resident batch and every earlier result stay as they are.

static const uint8_t BGZF_EOF_BLOCK[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

void moni_bgzf_params_default(moni_bgzf_params_t* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->block_size = BGZF_MAX_BLOCK; p->level = 1;
}

// The blocks of `len` bytes of text that are on the device already (the BAM path's records; moni_bgzf_compress after its upload): the kernels, the
// transfer into the pinned buffer, the end-of-file block.  st: everything but t_total, which is the caller's.
static int bgzf_compress_device(moni_ctx_t* c, const uint8_t* d_text, uint64_t len, const moni_bgzf_params_t* prm, const uint8_t** out, uint64_t* out_len,
                                moni_bgzf_stats_t& st) {
    auto& B = c->bz;
    const uint64_t nb = (len + prm->block_size - 1) / prm->block_size;
    const uint64_t slot = bgzf_slot_bytes(prm->block_size), bound = len + BGZF_FRAME * nb;          // every block stored: the most there can be
    const unsigned grid = (unsigned)std::min<uint64_t>(nb, (uint64_t)ctx_n_cu(c) * 4);          // 40 KB of LDS each: four workgroups share a CU
    int rc;
    if ((rc = B.h_out.ensure(bound + sizeof BGZF_EOF_BLOCK))) return rc;
    if (nb) {
        if ((rc = B.staging.ensure(nb * slot / 4)) || (rc = B.tok.ensure((uint64_t)grid * BGZF_MAX_BLOCK)) || (rc = B.out.ensure(bound)) ||
            (rc = B.len.ensure(nb + 1)) || (rc = B.off.ensure(nb + 1)) || (rc = B.pos.ensure(nb + 1)) || (rc = B.counters.ensure(4)) || (rc = B.h_sum.ensure(8)))
            return rc;
        if (!B.e0.h) HIPCHK(hipEventCreate(&B.e0.h));
        if (!B.e1.h) HIPCHK(hipEventCreate(&B.e1.h));
    }
    memset(&st, 0, sizeof st);
    st.in_bytes = len;
    uint64_t total = 0;
    if (nb) {
        HIPCHK(hipMemsetAsync(B.staging.p, 0, nb * slot, c->stream));
        HIPCHK(hipMemsetAsync(B.counters.p, 0, 4 * sizeof(unsigned long long), c->stream));
        HIPCHK(hipMemsetAsync(B.len.p + nb, 0, sizeof(uint64_t), c->stream));          // the scan's last entry: the sum
        bgzf_args_t G;
        G.text = d_text; G.len = len; G.block_size = prm->block_size; G.level = prm->level; G.n_blocks = nb;
        G.staging = B.staging.p; G.tok = B.tok.p; G.out_len = B.len.p; G.out_off = B.off.p; G.counters = B.counters.p;
        HIPCHK(hipEventRecord(B.e0, c->stream));
        hipLaunchKernelGGL(bgzf_block_kernel, dim3(grid), dim3(BGZF_T), 0, c->stream, G);
        if ((rc = exclusive_scan_u64(c, B.len.p, B.pos.p, nb + 1))) return rc;
        hipLaunchKernelGGL(gather_lines_kernel, dim3((unsigned)std::min<uint64_t>((nb + 3) / 4, (uint64_t)ctx_n_cu(c) * 8)), dim3(256), 0, c->stream,
                           (const uint64_t*)B.staging.p, (const uint64_t*)B.len.p, (const uint64_t*)B.off.p, (const uint64_t*)B.pos.p, nb, B.out.p);
        HIPCHK(hipEventRecord(B.e1, c->stream));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(B.h_sum.p, B.pos.p + nb, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(B.h_sum.p + 1, B.counters.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        total = B.h_sum.p[0];
        if (total > bound || B.h_sum.p[4]) { fprintf(stderr, "moni_hip: bgzf: the blocks' sizes are inconsistent\n"); return MONI_ERANGE; }
        HIPCHK(hipMemcpyAsync(B.h_out.p, B.out.p, total, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, B.e0, B.e1));
        st.t_kernel = ms * 1e-3;
        st.matches = B.h_sum.p[1]; st.literals = B.h_sum.p[2]; st.stored_blocks = B.h_sum.p[3];
    }
    if (prm->eof) { memcpy(B.h_out.p + total, BGZF_EOF_BLOCK, sizeof BGZF_EOF_BLOCK); total += sizeof BGZF_EOF_BLOCK; }
    st.out_bytes = total; st.blocks = nb + (prm->eof ? 1 : 0);
    *out = B.h_out.p; *out_len = total;
    return MONI_OK;
}

int moni_bgzf_compress(moni_ctx_t* c, const void* text, uint64_t len, const moni_bgzf_params_t* prm, const uint8_t** out, uint64_t* out_len,
                       moni_bgzf_stats_t* stats) {
    if (!c || !prm || !out || !out_len || !bgzf_params_ok(*prm) || (!text && len)) return MONI_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(c->idx->device));
    int rc;
    if (len) {
        if ((rc = c->bz.text.ensure(len))) return rc;
        HIPCHK(hipMemcpyAsync(c->bz.text.p, text, len, hipMemcpyHostToDevice, c->stream));
    }
    moni_bgzf_stats_t st;
    if ((rc = bgzf_compress_device(c, c->bz.text.p, len, prm, out, out_len, st))) return rc;
    st.t_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = st;
    return MONI_OK;
}
