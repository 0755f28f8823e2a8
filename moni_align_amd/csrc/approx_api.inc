// Host side of the k-mismatch queries (included inside extern "C" of moni_hip.hip): the kernels are in approx_kernels.hip.
// One run = pack_kernel, then - with k >= 1 - approx_plan_kernel and the rocPRIM exclusive scan of the chunk counts; approx_exact_kernel (pass 1);
// approx_tree_kernel (pass 2, k >= 1); with max_hits > 0 approx_finish_kernel, the scan of the kept counts, one 8-byte copy of their total,
// approx_gather_kernel, and with max_occ > 0 the scan of the hits' position counts, one 8-byte copy and approx_walk_kernel.  Nothing is launched for
// a phase with no work; the results stay on the device until fetched, where the hits of a task are put into their order.

void moni_approx_params_default(moni_approx_params_t* p) {
    if (!p) return;
    p->strands = 1; p->k = 1; p->max_hits = 0; p->max_occ = 0; p->chunk_len = MONI_APPROX_CHUNK_LEN_DEFAULT; p->reserved = 0; p->max_steps = MONI_APPROX_MAX_STEPS_DEFAULT;
}

static int approx_params_ok(const moni_approx_params_t* p) {
    return p && (p->strands == 1 || p->strands == 2) && p->k <= MONI_APPROX_MAX_K && p->chunk_len >= 1 && !p->reserved && !(p->max_occ && !p->max_hits);
}

static int approx_run_resident(moni_ctx* c, const moni_approx_params_t* prm) {
    moni_index* I = c->idx;
    SearchDims D; int rc;
    if ((rc = search_dims(c, prm->strands, D))) return rc;
    auto& B = c->apx;
    B.valid = false;
    const uint64_t nr = D.nr, n_tasks = D.n_tasks;
    const unsigned task_grid = D.task_grid;
    if (prm->max_hits && n_tasks > (~0ull >> 8) / prm->max_hits) return MONI_ENOMEM;          // the hit region's size in bytes does not fit 62 bits
    const uint64_t n_slots = n_tasks * prm->max_hits;
    const uint64_t ck_bound = prm->k ? prm->strands * (c->total_len / prm->chunk_len) + n_tasks : 0;      // sum of ceil(m / chunk_len) at most
    if ((rc = B.slots.ensure(n_slots + 1)) || (rc = B.res.ensure(n_tasks + 1)) || (rc = B.cnt.ensure(n_tasks + 2)) || (rc = B.ck_off.ensure(n_tasks + 2)) ||
        (rc = B.hit_off.ensure(n_tasks + 2)) || (rc = B.ckpt.ensure(ck_bound + 1)))
        return refused(rc);
    if ((rc = search_pack(c, D))) return rc;          // (before A: it places the patterns' workspace)
    apx_args_t A;
    A.rows = I->d_rows.p; A.frows = I->d_frows.p; A.cr = I->d_cr.p; A.recs = I->d_recs.p; A.pat = c->pat.p; A.offs = c->offs.p; A.blk = c->blk.p;
    A.strands = prm->strands; A.k = prm->k; A.max_hits = prm->max_hits; A.max_occ = prm->max_occ; A.chunk_len = prm->chunk_len; A.max_steps = prm->max_steps;
    A.res = B.res.p; A.slots = B.slots.p;
    if (nr) {
        if (prm->k) {
            hipLaunchKernelGGL(approx_plan_kernel, dim3(task_grid), dim3(MS_BLOCK), 0, c->stream, c->offs.p, n_tasks, prm->strands, prm->chunk_len, B.cnt.p);
            HIPCHK(hipGetLastError());
            if ((rc = exclusive_scan_u64(c, B.cnt.p, B.ck_off.p, n_tasks + 1))) return rc;
        }
    }
    rec(c, EV_MS0);
    if (nr)
        hipLaunchKernelGGL(approx_exact_kernel, dim3(task_grid), dim3(MS_BLOCK), 0, c->stream, I->K, I->d_tables.p, A, n_tasks, prm->k ? B.ck_off.p : nullptr,
                           prm->k ? B.ckpt.p : nullptr, c->d_counters.p);
    rec(c, EV_MS1);
    HIPCHK(hipGetLastError());
    rec(c, EV_PC0);
    uint64_t n_hits = 0, n_occ = 0;
    if (nr && prm->k && ck_bound) {
        const uint64_t blocks = (ck_bound + MS_BLOCK - 1) / MS_BLOCK;
        hipLaunchKernelGGL(approx_tree_kernel, dim3((unsigned)std::min<uint64_t>(blocks, APX_MAX_GRID)), dim3(MS_BLOCK), 0, c->stream, I->K, I->d_tables.p, A, n_tasks, B.ck_off.p,
                           B.ckpt.p, c->d_counters.p);
        HIPCHK(hipGetLastError());
    }
    if (nr && prm->max_hits) {
        hipLaunchKernelGGL(approx_finish_kernel, dim3(task_grid), dim3(MS_BLOCK), 0, c->stream, n_tasks, prm->max_hits, B.res.p, B.cnt.p);
        HIPCHK(hipGetLastError());
        if ((rc = exclusive_scan_u64(c, B.cnt.p, B.hit_off.p, n_tasks + 1))) return rc;
        HIPCHK(hipMemcpyAsync(&n_hits, B.hit_off.p + n_tasks, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (n_hits) {
        if ((rc = B.hits.ensure(n_hits + 1)) || (rc = B.occ_cnt.ensure(n_hits + 2)) || (rc = B.occ_off.ensure(n_hits + 2))) return refused(rc);
        hipLaunchKernelGGL(approx_gather_kernel, dim3((unsigned)((n_slots + MS_BLOCK - 1) / MS_BLOCK)), dim3(MS_BLOCK), 0, c->stream, n_tasks, prm->max_hits, B.res.p, B.hit_off.p,
                           prm->max_occ ? 1u : 0u, B.slots.p, B.hits.p, B.occ_cnt.p);
        HIPCHK(hipGetLastError());
        if (prm->max_occ) {
            if ((rc = exclusive_scan_u64(c, B.occ_cnt.p, B.occ_off.p, n_hits + 1))) return rc;
            HIPCHK(hipMemcpyAsync(&n_occ, B.occ_off.p + n_hits, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
    }
    rec(c, EV_PC1);
    rec(c, EV_PE0);
    if (n_occ) {
        if ((rc = B.pos.ensure(n_occ)) || (rc = B.seq.ensure(n_occ)) || (rc = B.seq_off.ensure(n_occ))) return refused(rc);
        phi_tab_t P; P.recs = I->d_phi.p; P.dir = I->d_phi_dir.p;
        hipLaunchKernelGGL(approx_walk_kernel, dim3((unsigned)((n_hits + MS_BLOCK - 1) / MS_BLOCK)), dim3(MS_BLOCK), 0, c->stream, I->K, P, I->d_seq_starts.p, n_hits, B.hits.p,
                           B.occ_off.p, B.pos.p, B.seq.p, B.seq_off.p, c->d_counters.p);
    }
    rec(c, EV_PE1);
    rec(c, EV_ALL1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    B.n_tasks = n_tasks; B.n_hits = n_hits; B.n_occ = n_occ; B.valid = true;
    return MONI_OK;
}

int moni_approx_run(moni_ctx_t* c, const moni_approx_params_t* prm) {
    if (!c || !approx_params_ok(prm)) return MONI_EINVAL;
    return approx_run_resident(c, prm);
}

int moni_approx_sizes(moni_ctx_t* c, uint64_t* n_tasks, uint64_t* n_hits_kept, uint64_t* n_occ) {
    if (!c || !c->apx.valid) return MONI_EINVAL;
    if (n_tasks) *n_tasks = c->apx.n_tasks;
    if (n_hits_kept) *n_hits_kept = c->apx.n_hits;
    if (n_occ) *n_occ = c->apx.n_occ;
    return MONI_OK;
}

int moni_approx_fetch(moni_ctx_t* c, moni_approx_res_t* res, moni_approx_hit_t* hits, uint64_t* pos, uint32_t* seq, uint64_t* seq_off) {
    if (!c || !c->apx.valid) return MONI_EINVAL;
    HIPCHK(hipSetDevice(c->idx->device));
    const auto& B = c->apx;
    try {
        std::vector<moni_approx_res_t> hres(B.n_tasks);
        if (B.n_tasks) HIPCHK(hipMemcpy(hres.data(), B.res.p, B.n_tasks * sizeof(moni_approx_res_t), hipMemcpyDeviceToHost));
        if (res && B.n_tasks) memcpy(res, hres.data(), B.n_tasks * sizeof(moni_approx_res_t));
        if (!hits || !B.n_hits) return MONI_OK;
        HIPCHK(hipMemcpy(hits, B.hits.p, B.n_hits * sizeof(moni_approx_hit_t), hipMemcpyDeviceToHost));
        apx_sort_hits(hits, hres.data(), B.n_tasks);
        // the positions follow their hits: the device wrote them in the order the lanes took their slots
        std::vector<uint64_t> tp, to; std::vector<uint32_t> ts;
        if (B.n_occ && pos) { tp.resize(B.n_occ); HIPCHK(hipMemcpy(tp.data(), B.pos.p, B.n_occ * sizeof(uint64_t), hipMemcpyDeviceToHost)); }
        if (B.n_occ && seq) { ts.resize(B.n_occ); HIPCHK(hipMemcpy(ts.data(), B.seq.p, B.n_occ * sizeof(uint32_t), hipMemcpyDeviceToHost)); }
        if (B.n_occ && seq_off) { to.resize(B.n_occ); HIPCHK(hipMemcpy(to.data(), B.seq_off.p, B.n_occ * sizeof(uint64_t), hipMemcpyDeviceToHost)); }
        uint64_t at = 0;
        for (uint64_t h = 0; h < B.n_hits; ++h) {
            const uint64_t from = hits[h].occ_off, k = hits[h].n_occ;
            if (!tp.empty()) std::copy(tp.begin() + from, tp.begin() + from + k, pos + at);
            if (!ts.empty()) std::copy(ts.begin() + from, ts.begin() + from + k, seq + at);
            if (!to.empty()) std::copy(to.begin() + from, to.begin() + from + k, seq_off + at);
            hits[h].occ_off = at;
            at += k;
        }
    } catch (const std::bad_alloc&) { return MONI_ENOMEM; }
    return MONI_OK;
}

int moni_approx_batch(moni_ctx_t* c, const moni_read_batch_t* b, const moni_approx_params_t* prm, moni_approx_res_t* res, moni_approx_hit_t** hits, uint64_t** pos,
                      uint32_t** seq, uint64_t** seq_off, uint64_t* n_hits_kept, uint64_t* n_occ) {
    if (!c || !b || !approx_params_ok(prm)) return MONI_EINVAL;
    if (hits) *hits = nullptr;
    if (pos) *pos = nullptr;
    if (seq) *seq = nullptr;
    if (seq_off) *seq_off = nullptr;
    if (n_hits_kept) *n_hits_kept = 0;
    if (n_occ) *n_occ = 0;
    int rc = moni_reads_upload(c, b);
    if (rc) return rc;
    if (!b->n_reads) return MONI_OK;
    if ((rc = approx_run_resident(c, prm))) return rc;
    const uint64_t nh = c->apx.n_hits, n = c->apx.n_occ;
    HostArrays H;
    moni_approx_hit_t* hh = H.want(hits, nh);          // without the hits their positions have no owner: none is fetched
    const uint64_t np = hh ? n : 0;
    uint64_t* hp = H.want(pos, np); uint32_t* hs = H.want(seq, np); uint64_t* ho = H.want(seq_off, np);
    if (!H.ok) return MONI_ENOMEM;
    if ((rc = moni_approx_fetch(c, res, hh, hp, hs, ho))) return rc;
    H.release();
    if (n_hits_kept) *n_hits_kept = hh ? nh : 0;
    if (n_occ) *n_occ = np;
    return MONI_OK;
}
