"""Life cycle of the library's handles: every device and pinned buffer, stream and event of an index and a context belongs to a member that frees
it (moni_align_amd/csrc/owned_buf.hpp), so creating, using and destroying them in any order must neither fault nor change a result.  The tests
run every query mode on a small index, destroy contexts with results unfetched and batches parked, regrow the context's text buffer, and compare
every output with the same call in a fresh context.  Parity checks: no tolerance."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MONI_EINVAL = -22


def _ragged(items):
    offs = np.zeros(len(items) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in items])
    return np.frombuffer(b"".join(items), dtype=np.uint8).copy(), offs


class Batch:
    """n simulated reads of length L with names and qualities, in the layout the library takes"""

    def __init__(self, case, n, L, seed):
        reads = case.synth.make_reads(case.pg, n, L, seed=seed, sub_rate=0.02, indel_rate=0.002)
        self.seq = reads.reshape(-1).copy()
        self.offs = np.arange(0, (n + 1) * L, L, dtype=np.uint64)
        self.names, self.noff = case.synth.make_names(n, prefix="s%d" % seed)
        self.quals = np.random.default_rng(seed).integers(35, 74, size=n * L).astype(np.uint8)


@pytest.fixture(scope="module")
def inputs(small_case):
    """what one cycle runs: 48 reads, 24 pairs, 24 exact patterns cut from the first haplotype (they occur in the others too)"""
    case = small_case
    reads = Batch(case, 48, 100, 21)
    mates, _ = case.synth.make_pairs(case.pg, 24, 100, seed=22)
    pnames = [b"p%d/%d" % (i, k + 1) for i in range(24) for k in range(2)]
    s0 = case.pg.seqs[0].tobytes()
    pats = [s0[97 * k + 5: 97 * k + 5 + 20 + k] for k in range(24)]
    return {"reads": reads, "pseq": mates.reshape(-1).copy(), "poffs": np.arange(0, 49 * 100, 100, dtype=np.uint64), "pnames": _ragged(pnames),
            "pq": np.full(48 * 100, ord("I"), np.uint8), "pats": _ragged(pats)}


def _pe_model():
    from moni_align_amd import capi
    m = capi.PeModelC()
    m.mean, m.std_dev, m.complete = 350.0, 30.0, 1          # (24 pairs do not complete the learning: the model make_pairs draws from)
    return m


def _cycle(case, inp):
    """an index and a context, every mode once, both closed; the outputs by name"""
    from moni_align_amd import capi
    r = inp["reads"]
    idx = capi.Index(fi=case.fi, device=0)
    ctx = capi.Ctx(idx)
    out = {}
    try:
        out["ms_query"] = ctx.ms_query_batch(r.seq, r.offs)
        ctx.upload(r.seq, r.offs)
        ctx.seed_run(25, True, 1000)
        seeds = ctx.seed_fetch()
        out["mems"], out["occs"], out["read_mem_off"] = seeds["mems"], seeds["occs"], seeds["read_mem_off"]
        out["align"] = ctx.align_batch(r.seq, r.offs, r.names, r.noff, r.quals, host_threads=2)[0]
        out["pe_align"] = ctx.pe_align(inp["pseq"], inp["poffs"], *inp["pnames"], inp["pq"], _pe_model(), host_threads=2)[0]
        out["extend"] = ctx.extend_batch(r.seq, r.offs, r.names, r.noff, r.quals)[0]
        out["pml_len"], out["pml_max"], out["pml_hits"] = ctx.pml_batch(r.seq, r.offs)
        for k, v in zip(("res", "pos", "seq", "seq_off"), ctx.locate_batch(*inp["pats"], strands=2, max_occ=4)):
            out["locate_" + k] = v
        out["seqcount_res"], out["seqcount_counts"] = ctx.seqcount_batch(*inp["pats"], strands=2)
        for k, v in zip(("res", "hits", "pos", "seq", "seq_off"), ctx.approx_batch(*inp["pats"], strands=1, k=1, max_hits=8, max_occ=4)):
            out["approx_" + k] = v
        out["mslong_ptr"], out["mslong_len"], _ = ctx.ms_long_batch(r.seq, r.offs)
    finally:
        ctx.close()
        idx.close()
    return out


def _same(a, b):
    if isinstance(a, bytes):
        return a == b
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.names:          # records: field by field (the bytes between the fields are nobody's)
        return all(np.array_equal(a[f], b[f]) for f in a.dtype.names)
    return a.tobytes() == b.tobytes()


def test_create_run_destroy_cycles(small_case, inputs):
    """four cycles of (index, context, every query mode once, destroy): the fourth cycle's outputs are the first's, byte for byte.  The device
    memory that is free after cycle 1 and after cycle 4 is printed, not asserted: other processes share the GPU."""
    import torch
    torch.cuda.mem_get_info()          # (the first call sets up torch's own context: not part of the difference)
    first = last = None
    free = {}
    for cyc in range(1, 5):
        out = _cycle(small_case, inputs)
        if cyc == 1:
            first = out
        last = out
        if cyc in (1, 4):
            free[cyc] = torch.cuda.mem_get_info()[0]
    print("device memory free after cycle 1: %d bytes, after cycle 4: %d bytes, drift (cycle 1 - cycle 4): %d bytes" % (free[1], free[4], free[1] - free[4]))
    assert len(first["align"]) > 0 and len(first["pe_align"]) > 0 and len(first["extend"]) > 0 and len(first["mems"]) > 0
    assert int(first["locate_res"]["count"].sum()) > 0 and len(first["locate_pos"]) > 0 and len(first["approx_hits"]) > 0 and len(first["approx_pos"]) > 0
    assert int(first["seqcount_counts"].sum()) > 0
    assert sorted(first) == sorted(last)
    for k in first:
        assert _same(first[k], last[k]), k


def _locate_sizes_rc(ctx):
    nt, no = ctypes.c_uint64(), ctypes.c_uint64()
    return ctx._L.moni_locate_sizes(ctx._h, ctypes.byref(nt), ctypes.byref(no))


def test_destroy_with_results_pending(small_case, inputs):
    """results of locate, seqcount and approx left unfetched when the context goes; and the one place that invalidates them: after a new batch is
    made resident - by upload or by swap - moni_locate_sizes gives MONI_EINVAL"""
    from moni_align_amd import capi
    idx = capi.Index(fi=small_case.fi, device=0)
    try:
        ctx = capi.Ctx(idx)
        ctx.upload(*inputs["pats"])
        ctx.locate_run(strands=2, max_occ=4)
        ctx.seqcount_run(strands=2)
        ctx.approx_run(strands=1, k=1, max_hits=8, max_occ=4)
        ctx.close()
        ctx = capi.Ctx(idx)
        try:
            seq, offs = inputs["pats"]
            assert _locate_sizes_rc(ctx) == MONI_EINVAL          # before any run
            ctx.upload(seq, offs)
            ctx.locate_run(strands=1, max_occ=2)
            assert _locate_sizes_rc(ctx) == 0
            ctx.upload(seq[: int(offs[5])], offs[:6])
            assert _locate_sizes_rc(ctx) == MONI_EINVAL
            ctx.locate_run(strands=1, max_occ=2)
            assert _locate_sizes_rc(ctx) == 0
            ctx.swap(0)
            assert _locate_sizes_rc(ctx) == MONI_EINVAL
        finally:
            ctx.close()
    finally:
        idx.close()


def test_swap_then_destroy(small_case):
    """three batches parked in slots 0, 1, 2; the one of slot 1 comes back and aligns as in a fresh context; the context goes with two still parked"""
    from moni_align_amd import capi
    batches = [Batch(small_case, n, L, seed) for n, L, seed in ((40, 100, 31), (33, 150, 32), (64, 75, 33))]
    idx = capi.Index(fi=small_case.fi, device=0)
    try:
        ctx = capi.Ctx(idx)
        try:
            for slot, b in enumerate(batches):
                ctx.upload(b.seq, b.offs)
                ctx.swap(slot)
            assert ctx.n_reads == 0
            ctx.swap(1)
            b = batches[1]
            assert ctx.n_reads == len(b.offs) - 1
            got = ctx.align_run(b.names, b.noff, b.quals, host_threads=2)[0]
        finally:
            ctx.close()          # batches 0 and 2 parked
        ctx = capi.Ctx(idx)
        try:
            ctx.upload(b.seq, b.offs)
            want = ctx.align_run(b.names, b.noff, b.quals, host_threads=2)[0]
        finally:
            ctx.close()
    finally:
        idx.close()
    assert got.count(b"\n") == 33 and got == want


def test_out_buffer_regrows_and_keeps_text(small_case, monkeypatch):
    """the context's pinned text buffer: a small align_run, then one with fifty times the text (the buffer is replaced), then extend in chunks of 16
    reads; every text equals the same call's in a fresh context - where extend starts from an empty buffer and regrows it chunk after chunk with the
    text so far kept"""
    from moni_align_amd import capi
    monkeypatch.setenv("MONI_EXTEND_CHUNK", "16")
    small, large = Batch(small_case, 8, 100, 41), Batch(small_case, 400, 150, 42)
    idx = capi.Index(fi=small_case.fi, device=0)

    def fresh(fn):
        c = capi.Ctx(idx)
        try:
            return fn(c)
        finally:
            c.close()

    def align(b):
        def run(c):
            c.upload(b.seq, b.offs)
            return c.align_run(b.names, b.noff, b.quals, host_threads=2)[0]
        return run

    def extend(c):
        c.upload(large.seq, large.offs)
        return c.extend_run(large.names, large.noff, large.quals)[0]

    try:
        ctx = capi.Ctx(idx)
        try:
            got = [align(small)(ctx), align(large)(ctx), extend(ctx)]
        finally:
            ctx.close()
        want = [fresh(align(small)), fresh(align(large)), fresh(extend)]
    finally:
        idx.close()
    assert got[0].count(b"\n") == 8 and got[1].count(b"\n") == 400 and len(got[1]) > 20 * len(got[0]) and got[2].count(b"\n") >= 300
    assert got == want


QUERY_MODES = {          # run and fetch of the four pattern queries that share the search prologue, the patterns' workspace and the counters
    "locate": (lambda c, s: c.locate_run(strands=s, max_occ=4), lambda c: c.locate_fetch()),
    "seqcount": (lambda c, s: c.seqcount_run(strands=s), lambda c: c.seqcount_fetch()),
    "loci": (lambda c, s: c.loci_run(strands=s), lambda c: c.loci_fetch()),
    "approx": (lambda c, s: c.approx_run(strands=s, k=1, max_hits=4, max_occ=4), lambda c: c.approx_fetch()),
}


@pytest.mark.parametrize("strands", [1, 2])
def test_pattern_queries_keep_to_their_own_results(small_case, strands):
    """129 patterns on one context - 129 tasks at one strand, 258 at two: a 256-thread block and one thread, or one block and two threads - among
    them one that occurs nowhere and one with a byte outside ACGT.  locate, seq-count, loci and approx run in two orders; after every run its
    fetch, and after the last run of an order the fetch of all four, equal what the same mode returns in a context that ran nothing else."""
    from moni_align_amd import capi
    s0 = small_case.pg.seqs[0].tobytes()
    pats = [s0[29 * k + 3: 29 * k + 3 + 16 + k % 9] for k in range(127)]
    absent = b"ACGTTGCA" * 4
    assert absent not in small_case.text
    pats += [absent, s0[500:510] + b"N" + s0[511:524]]
    seq, offs = _ragged(pats)
    idx = capi.Index(fi=small_case.fi, device=0)
    try:
        want = {}
        for name, (run, fetch) in QUERY_MODES.items():
            ctx = capi.Ctx(idx)
            try:
                ctx.upload(seq, offs)
                run(ctx, strands)
                want[name] = fetch(ctx)
            finally:
                ctx.close()
        assert len(want["locate"][0]) == 129 * strands and int(want["locate"][0]["count"][: 127 * strands: strands].min()) > 0
        assert not want["locate"][0]["count"][127 * strands:].any() and len(want["locate"][1]) > 0 and len(want["approx"][1]) > 0
        assert int(want["seqcount"][1].sum()) > 0 and len(want["loci"][1]) > 0
        ctx = capi.Ctx(idx)
        try:
            ctx.upload(seq, offs)
            for order in (("locate", "seqcount", "loci", "approx"), ("approx", "loci", "locate", "seqcount")):
                for name in order:
                    QUERY_MODES[name][0](ctx, strands)
                    assert all(_same(g, w) for g, w in zip(QUERY_MODES[name][1](ctx), want[name])), (order, name)
                for name in order:
                    assert all(_same(g, w) for g, w in zip(QUERY_MODES[name][1](ctx), want[name])), (order, name, "after the order's last run")
        finally:
            ctx.close()
    finally:
        idx.close()
