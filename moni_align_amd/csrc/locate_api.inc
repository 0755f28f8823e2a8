// Host side of the exact-match queries (included inside extern "C" of moni_hip.hip): the kernels are in locate_kernels.hip.
// One run = pack_kernel (the patterns of the resident batch into the workspace) + count_kernel, then - with max_occ > 0 - the rocPRIM exclusive scan
// of the capped counts and locate_walk_kernel; the results stay on the device until fetched.

void moni_locate_params_default(moni_locate_params_t* p) {
    if (!p) return;
    p->strands = 1; p->max_occ = 0; p->reserved[0] = p->reserved[1] = 0;
}

static int locate_params_ok(const moni_locate_params_t* p) { return p && (p->strands == 1 || p->strands == 2) && !p->reserved[0] && !p->reserved[1]; }

static int locate_run_resident(moni_ctx* c, const moni_locate_params_t* prm) {
    moni_index* I = c->idx;
    HIPCHK(hipSetDevice(I->device));
    if (c->h_blk.empty()) return MONI_EINVAL;          // no batch was made resident
    auto& B = c->loc;
    B.valid = false;
    const uint64_t nr = c->n_reads, n_pack = 2 * nr, n_tasks = nr * prm->strands;
    int rc;
    if ((rc = c->pat.ensure(c->h_blk.back().y + 1)) || (rc = c->pflag.ensure(n_pack + 8)) || (rc = B.res.ensure(n_tasks + 1)) || (rc = B.toe.ensure(n_tasks + 1)) ||
        (rc = B.cnt.ensure(n_tasks + 2)) || (rc = B.off.ensure(n_tasks + 2)))
        return rc;
    HIPCHK(hipMemsetAsync(c->d_counters.p, 0, 4 * sizeof(unsigned long long), c->stream));
    rec(c, EV_ALL0);
    if (nr)
        hipLaunchKernelGGL(pack_kernel, dim3((unsigned)((n_pack + MS_BLOCK - 1) / MS_BLOCK)), dim3(MS_BLOCK), 0, c->stream, I->K, I->d_tables.p, c->seq.p, c->offs.p, c->blk.p, n_pack,
                           c->pat.p, c->pflag.p);
    rec(c, EV_MS0);
    if (nr)          // (one thread more than tasks: it closes the counts for the scan)
        hipLaunchKernelGGL(count_kernel, dim3((unsigned)((n_tasks + 1 + MS_BLOCK - 1) / MS_BLOCK)), dim3(MS_BLOCK), 0, c->stream, I->K, I->d_tables.p, I->d_rows.p, I->d_frows.p, I->d_cr.p,
                           I->d_recs.p, c->pat.p, c->offs.p, c->blk.p, n_tasks, prm->strands, prm->max_occ, B.res.p, B.toe.p, B.cnt.p, c->d_counters.p);
    rec(c, EV_MS1);
    HIPCHK(hipGetLastError());
    uint64_t total = 0;
    if (nr && prm->max_occ) {
        if ((rc = exclusive_scan_u64(c, B.cnt.p, B.off.p, n_tasks + 1))) return rc;
        HIPCHK(hipMemcpyAsync(&total, B.off.p + n_tasks, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    rec(c, EV_PC0);
    if (total) {          // no occurrence to list: no walk launch
        if ((rc = B.pos.ensure(total)) || (rc = B.seq.ensure(total)) || (rc = B.seq_off.ensure(total))) return rc;
        phi_tab_t P; P.recs = I->d_phi.p; P.dir = I->d_phi_dir.p;
        hipLaunchKernelGGL(locate_walk_kernel, dim3((unsigned)((n_tasks + MS_BLOCK - 1) / MS_BLOCK)), dim3(MS_BLOCK), 0, c->stream, I->K, P, I->d_seq_starts.p, n_tasks, B.res.p, B.toe.p,
                           B.off.p, B.pos.p, B.seq.p, B.seq_off.p, c->d_counters.p);
    }
    rec(c, EV_PC1);
    rec(c, EV_ALL1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    B.n_tasks = n_tasks; B.n_occ = total; B.valid = true;
    return MONI_OK;
}

int moni_locate_run(moni_ctx_t* c, const moni_locate_params_t* prm) {
    if (!c || !locate_params_ok(prm)) return MONI_EINVAL;
    return locate_run_resident(c, prm);
}

int moni_locate_sizes(moni_ctx_t* c, uint64_t* n_tasks, uint64_t* n_occ) {
    if (!c || !c->loc.valid) return MONI_EINVAL;
    if (n_tasks) *n_tasks = c->loc.n_tasks;
    if (n_occ) *n_occ = c->loc.n_occ;
    return MONI_OK;
}

int moni_locate_fetch(moni_ctx_t* c, moni_locate_res_t* res, uint64_t* pos, uint32_t* seq, uint64_t* seq_off) {
    if (!c || !c->loc.valid) return MONI_EINVAL;
    HIPCHK(hipSetDevice(c->idx->device));
    const auto& B = c->loc;
    if (res && B.n_tasks) HIPCHK(hipMemcpy(res, B.res.p, B.n_tasks * sizeof(moni_locate_res_t), hipMemcpyDeviceToHost));
    if (pos && B.n_occ) HIPCHK(hipMemcpy(pos, B.pos.p, B.n_occ * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (seq && B.n_occ) HIPCHK(hipMemcpy(seq, B.seq.p, B.n_occ * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (seq_off && B.n_occ) HIPCHK(hipMemcpy(seq_off, B.seq_off.p, B.n_occ * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return MONI_OK;
}

int moni_locate_batch(moni_ctx_t* c, const moni_read_batch_t* b, const moni_locate_params_t* prm, moni_locate_res_t* res, uint64_t** pos, uint32_t** seq,
                      uint64_t** seq_off, uint64_t* n_occ) {
    if (!c || !b || !locate_params_ok(prm)) return MONI_EINVAL;
    if (pos) *pos = nullptr;
    if (seq) *seq = nullptr;
    if (seq_off) *seq_off = nullptr;
    if (n_occ) *n_occ = 0;
    int rc = moni_reads_upload(c, b);
    if (rc) return rc;
    if (!b->n_reads) return MONI_OK;
    if ((rc = locate_run_resident(c, prm))) return rc;
    const uint64_t n = c->loc.n_occ;
    uint64_t* hp = nullptr; uint32_t* hs = nullptr; uint64_t* ho = nullptr;
    if (n) {
        if (pos) hp = (uint64_t*)malloc(n * sizeof(uint64_t));
        if (seq) hs = (uint32_t*)malloc(n * sizeof(uint32_t));
        if (seq_off) ho = (uint64_t*)malloc(n * sizeof(uint64_t));
        if ((pos && !hp) || (seq && !hs) || (seq_off && !ho)) rc = MONI_ENOMEM;
    }
    if (!rc) rc = moni_locate_fetch(c, res, hp, hs, ho);
    if (rc) { free(hp); free(hs); free(ho); return rc; }
    if (pos) *pos = hp;
    if (seq) *seq = hs;
    if (seq_off) *seq_off = ho;
    if (n_occ) *n_occ = n;
    return MONI_OK;
}
