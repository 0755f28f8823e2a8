"""ctypes binding of libmoni_hip.so (include/moni_hip.h).

Python is only the test/bench driver here; the product is the shared library.  There is no
Python or CPU implementation behind these calls: if the library is missing or no HIP device is
present the calls raise."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Dict, Optional

import numpy as np

# streams beyond the runtime's hardware queues share one (the paired path keeps ~11 busy): a default for processes that set none, before HIP initialises
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_PATH = os.environ.get("MONI_HIP_LIB") or os.path.join(CSRC, "libmoni_hip.so")      # override: kernel-variant sweeps

EXPORTS = [
    "moni_version", "moni_index_create", "moni_index_load", "moni_index_destroy", "moni_index_n", "moni_index_r",
    "moni_index_device_bytes", "moni_index_text", "moni_ctx_create", "moni_ctx_destroy", "moni_reads_upload", "moni_reads_swap", "moni_ms_run",
    "moni_ms_query_batch", "moni_seed_run", "moni_seed_counts", "moni_seed_fetch", "moni_seed_batch", "moni_free",
    "moni_phi_lcp_batch", "moni_extz_batch", "moni_last_kernel_ms", "moni_last_counters", "moni_seed_occ_stats",
    "moni_seed_prefilter", "moni_seed_prefilter_stats", "moni_ms_leap_stats", "moni_index_leap_table",
    "moni_align_params_default", "moni_align_batch", "moni_align_csv_batch", "moni_align_run", "moni_align_stream", "moni_sam_header",
    "moni_ldx_info", "moni_ldx_rewrite", "moni_ldx_lift_batch", "moni_ldx_write",
    "moni_ms_file_info", "moni_ms_file_read", "moni_ms_file_write", "moni_index_load_reference", "moni_ms_lengths_batch", "moni_report_mems_batch",
    "moni_pe_params_default", "moni_pe_learn_batch", "moni_pe_align_batch", "moni_pe_align_stream", "moni_pe_align_run", "moni_pe_align_csv_batch", "moni_pe_report_mems_batch",
    "moni_extend_params_default", "moni_extend_batch", "moni_extend_run",
    "moni_pml_batch", "moni_pml_run", "moni_pml_fetch", "moni_pml_sizes",
    "moni_screen_params_default", "moni_screen_run", "moni_screen_sizes", "moni_screen_fetch", "moni_screen_batch",
    "moni_locate_params_default", "moni_locate_run", "moni_locate_sizes", "moni_locate_fetch", "moni_locate_batch",
    "moni_seqcount_params_default", "moni_seqcount_run", "moni_seqcount_sizes", "moni_seqcount_fetch", "moni_seqcount_batch",
    "moni_loci_params_default", "moni_loci_run", "moni_loci_sizes", "moni_loci_fetch", "moni_loci_batch",
    "moni_approx_params_default", "moni_approx_run", "moni_approx_sizes", "moni_approx_fetch", "moni_approx_batch",
    "moni_mslong_params_default", "moni_ms_long_batch",
    "moni_bgzf_params_default", "moni_bgzf_compress",
    "moni_bam_params_default", "moni_bam_set_header", "moni_bam_records",
    "moni_bam_sorted_run", "moni_bam_sort", "moni_bam_merge_plan", "moni_bam_plan_free",
    "moni_bam_sorted_run_dup", "moni_bam_dup_resolve", "moni_bam_sort_marked",
    "moni_bai_create", "moni_bai_add", "moni_bai_finish", "moni_bai_destroy",
    "moni_inflate_params_default", "moni_bgzf_scan", "moni_bgzf_inflate",
    "moni_bamin_params_default", "moni_bam_in_reset", "moni_bam_in_feed",
    "moni_cov_params_default", "moni_cov_create", "moni_cov_destroy", "moni_cov_add", "moni_cov_add_sorted", "moni_cov_seal", "moni_cov_next", "moni_cov_windows",
    "moni_cov_test_set_counted",
]


def bgzf_scan(data):
    """moni_bgzf_scan (host only): (return code, members wholly within `data`, the bytes they take, the sum of their ISIZE)"""
    buf = np.frombuffer(data, dtype=np.uint8)
    n, used, ob = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = lib().moni_bgzf_scan(buf.ctypes.data if buf.size else None, buf.size, C.byref(n), C.byref(used), C.byref(ob))
    return rc, n.value, used.value, ob.value


class FlatIndexC(C.Structure):
    _fields_ = [("n", C.c_uint64), ("r", C.c_uint64), ("w", C.c_uint64), ("n_seq", C.c_uint64),
                ("F", C.c_void_p), ("heads", C.c_void_p), ("starts", C.c_void_p), ("ssa", C.c_void_p),
                ("esa", C.c_void_p), ("thr", C.c_void_p), ("slcp", C.c_void_p), ("text", C.c_void_p),
                ("seq_starts", C.c_void_p), ("seq_names", C.c_char_p),
                ("lift_second", C.c_void_p), ("lift_len", C.c_void_p), ("lift_ins_off", C.c_void_p), ("lift_ins", C.c_void_p),
                ("lift_del_off", C.c_void_p), ("lift_del", C.c_void_p)]


class ReadBatchC(C.Structure):
    _fields_ = [("seq", C.c_void_p), ("offsets", C.c_void_p), ("n_reads", C.c_uint64)]


class SeedParamsC(C.Structure):
    _fields_ = [("min_len", C.c_uint32), ("filter_seeds", C.c_uint32), ("n_seeds_thr", C.c_uint32),
                ("report_mems", C.c_uint32)]


class AlignParamsC(C.Structure):
    _fields_ = [("min_len", C.c_uint32), ("ext_len", C.c_uint32), ("check_k", C.c_uint32), ("region_dist", C.c_uint32),
                ("filter_seeds", C.c_uint32), ("n_seeds_thr", C.c_uint32), ("filter_freq", C.c_uint32), ("left_mem_check", C.c_uint32),
                ("freq_thr", C.c_double),
                ("smatch", C.c_int8), ("smismatch", C.c_int8), ("gapo", C.c_int8), ("gapo2", C.c_int8), ("gape", C.c_int8), ("gape2", C.c_int8),
                ("end_bonus", C.c_int32), ("w", C.c_int32), ("zdrop", C.c_int32),
                ("max_dist_x", C.c_int64), ("max_dist_y", C.c_int64), ("max_iter", C.c_int64), ("max_pred", C.c_int64),
                ("min_chain_score", C.c_int64), ("min_chain_length", C.c_int64),
                ("host_threads", C.c_uint32), ("reserved", C.c_uint32)]


class AlignStatsC(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("aligned", C.c_uint64), ("dp_tasks", C.c_uint64), ("dp_cells", C.c_uint64), ("dp_rounds", C.c_uint64),
                ("t_seed", C.c_double), ("t_chain", C.c_double), ("t_dp", C.c_double), ("t_host", C.c_double),
                ("t_dp_kernel", C.c_double), ("handed_back", C.c_uint64), ("dp_reused", C.c_uint64), ("dp_cells_reused", C.c_uint64),
                ("kernel_fallback", C.c_uint64), ("dp_ref_bytes", C.c_uint64),
                ("t_k_chain", C.c_double), ("t_k_dp", C.c_double), ("t_k_select", C.c_double), ("t_k_finish", C.c_double),
                ("handover_why", C.c_uint64 * 12), ("dp_cells_cut", C.c_uint64), ("dp_slots", C.c_uint64), ("runs_routed", C.c_uint64)]


class PeParamsC(C.Structure):
    _fields_ = [("filter_dir", C.c_uint32), ("find_orphan", C.c_uint32), ("dir_thr", C.c_double), ("ins_learning_n", C.c_uint64),
                ("ins_learning_score_gap_threshold", C.c_uint64), ("secondary_chains", C.c_uint32), ("reserved", C.c_uint32)]


class PeModelC(C.Structure):
    _fields_ = [("mean", C.c_double), ("std_dev", C.c_double), ("variance", C.c_double), ("sample_variance", C.c_double), ("m2", C.c_double),
                ("count", C.c_uint64), ("complete", C.c_uint32), ("reserved", C.c_uint32)]


class ExtendParamsC(C.Structure):
    _fields_ = [("min_len", C.c_uint32), ("ext_len", C.c_uint32),
                ("smatch", C.c_int8), ("smismatch", C.c_int8), ("gapo", C.c_int8), ("gape", C.c_int8),
                ("end_bonus", C.c_int32), ("w", C.c_int32), ("zdrop", C.c_int32), ("reserved", C.c_uint32)]


class ExtendStatsC(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("extended", C.c_uint64), ("records", C.c_uint64), ("dp_tasks", C.c_uint64), ("dp_cells", C.c_uint64),
                ("t_kernel", C.c_double)]


class ScreenParamsC(C.Structure):
    _fields_ = [("window", C.c_uint32), ("min_win", C.c_uint32), ("ks_num", C.c_uint32), ("ks_den", C.c_uint32), ("strands", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


class LocateParamsC(C.Structure):
    _fields_ = [("strands", C.c_uint32), ("max_occ", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class SeqcountParamsC(C.Structure):
    _fields_ = [("strands", C.c_uint32), ("reserved", C.c_uint32), ("max_walk", C.c_uint64)]


class LociParamsC(C.Structure):
    _fields_ = [("strands", C.c_uint32), ("lift", C.c_uint32), ("max_walk", C.c_uint64), ("max_total", C.c_uint64), ("reserved", C.c_uint64 * 2)]


class ApproxParamsC(C.Structure):
    _fields_ = [("strands", C.c_uint32), ("k", C.c_uint32), ("max_hits", C.c_uint32), ("max_occ", C.c_uint32), ("chunk_len", C.c_uint32), ("reserved", C.c_uint32),
                ("max_steps", C.c_uint64)]


class MslongParamsC(C.Structure):
    _fields_ = [("seg_len", C.c_uint32), ("overlap", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class MslongStatsC(C.Structure):
    _fields_ = [("patterns", C.c_uint64), ("bases", C.c_uint64), ("segments", C.c_uint64), ("flagged", C.c_uint64), ("chain_runs", C.c_uint64),
                ("steps_spec", C.c_uint64), ("steps_chain", C.c_uint64), ("jumps", C.c_uint64),
                ("t_walk", C.c_double), ("t_len", C.c_double), ("t_chain", C.c_double), ("t_total", C.c_double)]


class BgzfParamsC(C.Structure):
    _fields_ = [("block_size", C.c_uint32), ("level", C.c_uint32), ("eof", C.c_uint32), ("reserved", C.c_uint32)]


class BgzfStatsC(C.Structure):
    _fields_ = [("in_bytes", C.c_uint64), ("out_bytes", C.c_uint64), ("blocks", C.c_uint64), ("stored_blocks", C.c_uint64), ("matches", C.c_uint64),
                ("literals", C.c_uint64), ("t_kernel", C.c_double), ("t_total", C.c_double)]


class InflateParamsC(C.Structure):
    _fields_ = [("check_crc", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class InflateStatsC(C.Structure):
    _fields_ = [("in_bytes", C.c_uint64), ("out_bytes", C.c_uint64), ("blocks", C.c_uint64), ("bad_blocks", C.c_uint64), ("first_bad_block", C.c_uint64),
                ("bad_reason", C.c_uint32), ("pad", C.c_uint32), ("stored", C.c_uint64), ("fixed", C.c_uint64), ("dynamic", C.c_uint64),
                ("t_kernel", C.c_double), ("t_total", C.c_double)]


class BamInParamsC(C.Structure):
    _fields_ = [("paired", C.c_uint32), ("check_crc", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class BamInStatsC(C.Structure):
    _fields_ = [("inflate", InflateStatsC), ("records", C.c_uint64), ("reads", C.c_uint64), ("skipped_secondary", C.c_uint64), ("skipped_empty", C.c_uint64),
                ("carried_bytes", C.c_uint64), ("bad_records", C.c_uint64), ("first_bad_record", C.c_uint64), ("bad_record_reason", C.c_uint32),
                ("header_done", C.c_uint32), ("t_kernel", C.c_double * 4), ("t_total", C.c_double)]


BAMIN_REASONS = ("OK", "MAGIC", "HEADER", "BLOCK_SIZE", "FIELDS", "PAIRING", "TRUNCATED")
BAMIN_PHASES = ("inflate", "find", "select", "text")          # moni_bamin_stats_t::t_kernel
INF_REASONS = ("OK", "HEADER", "BTYPE", "STORED_LEN", "CODE_LENGTHS", "BAD_SYMBOL", "DISTANCE", "OVERRUN", "TRUNCATED", "TRAILING", "ISIZE", "CRC")


class BamParamsC(C.Structure):
    _fields_ = [("block_size", C.c_uint32), ("level", C.c_uint32), ("eof", C.c_uint32), ("raw", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class BamStatsC(C.Structure):
    _fields_ = [("in_bytes", C.c_uint64), ("lines", C.c_uint64), ("bam_bytes", C.c_uint64), ("out_bytes", C.c_uint64), ("blocks", C.c_uint64),
                ("bad_lines", C.c_uint64), ("first_bad_line", C.c_uint64), ("bad_reason", C.c_uint32), ("pad", C.c_uint32),
                ("t_encode", C.c_double), ("t_deflate", C.c_double), ("t_total", C.c_double)]


# moni_bam_stats_t::bad_reason (include/moni_hip.h: MONI_BAM_*)
BAM_REASONS = ("OK", "NEWLINE", "AT", "FIELDS", "QNAME", "INT", "RNAME", "CIGAR", "SEQ", "QUAL", "TAG", "TAGINT", "TAGTYPE", "LENGTH")


class BamBadLine(ValueError):
    """moni_bam_records met a bad line and wrote nothing: .stats holds bad_lines, first_bad_line and bad_reason"""

    def __init__(self, stats):
        self.stats = stats
        r = stats["bad_reason"]
        super().__init__("moni_bam_records: %d bad line(s), the first is line %d (%s)" %
                         (stats["bad_lines"], stats["first_bad_line"], BAM_REASONS[r] if r < len(BAM_REASONS) else r))


class BamSortStatsC(C.Structure):
    _fields_ = [("in_bytes", C.c_uint64), ("records", C.c_uint64), ("bam_bytes", C.c_uint64), ("out_bytes", C.c_uint64), ("blocks", C.c_uint64),
                ("bad_records", C.c_uint64), ("first_bad_record", C.c_uint64), ("bad_reason", C.c_uint32), ("pad", C.c_uint32),
                ("t_encode", C.c_double), ("t_key", C.c_double), ("t_sort", C.c_double), ("t_gather", C.c_double), ("t_deflate", C.c_double),
                ("t_total", C.c_double)]


class BamPlanC(C.Structure):
    _fields_ = [("n_chunks", C.c_uint64), ("n_runs", C.c_uint64), ("cuts", C.POINTER(C.c_uint64))]


# moni_bam_ent_t: an index entry of a sorted record
BAM_ENT_DTYPE = np.dtype([("ref_id", np.int32), ("pos", np.int32), ("end", np.int32), ("bin_flag", np.uint32), ("off", np.uint64)])
# moni_bam_sort_stats_t::bad_reason (include/moni_hip.h: MONI_BAMSORT_*)
BAMSORT_REASONS = ("OK", "OFFSET", "SHORT", "SIZE", "NAME", "REF", "POS", "LENGTH", "SEQ", "CLIP", "MATE")
# moni_bam_dup_t: an entry of duplicate marking
BAM_DUP_DTYPE = np.dtype([("k1", np.uint64), ("k2", np.uint64), ("score", np.uint32), ("kind", np.uint32), ("idx", np.uint32, (2,))])


class BamRunDupStatsC(C.Structure):
    _fields_ = [("run", BamSortStatsC), ("entries", C.c_uint64), ("pairs", C.c_uint64), ("fragments", C.c_uint64), ("bad_is_record", C.c_uint32), ("pad", C.c_uint32),
                ("t_sig", C.c_double), ("t_entry", C.c_double)]


class BamDupStatsC(C.Structure):
    _fields_ = [("entries", C.c_uint64), ("pairs", C.c_uint64), ("dup_pairs", C.c_uint64), ("fragments", C.c_uint64), ("dup_fragments", C.c_uint64),
                ("marked_records", C.c_uint64), ("bad_entries", C.c_uint64), ("first_bad_entry", C.c_uint64),
                ("t_sort", C.c_double), ("t_flag", C.c_double), ("t_total", C.c_double)]


class BamBadEntry(ValueError):
    """moni_bam_dup_resolve met an entry outside its run and wrote no mark: .stats holds bad_entries and first_bad_entry"""

    def __init__(self, stats):
        self.stats = stats
        super().__init__("moni_bam_dup_resolve: %d bad entr(ies), the first is entry %d" % (stats["bad_entries"], stats["first_bad_entry"]))


class BamBadRecord(ValueError):
    """moni_bam_sort met a bad record and wrote nothing: .stats holds bad_records, first_bad_record and bad_reason"""

    def __init__(self, stats):
        self.stats = stats
        r = stats["bad_reason"]
        super().__init__("moni_bam_sort: %d bad record(s), the first is record %d (%s)" %
                         (stats["bad_records"], stats["first_bad_record"], BAMSORT_REASONS[r] if r < len(BAMSORT_REASONS) else r))


class CovParamsC(C.Structure):
    _fields_ = [("exclude_flags", C.c_uint32), ("min_mapq", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class CovStatsC(C.Structure):
    _fields_ = [("records", C.c_uint64), ("counted", C.c_uint64), ("skipped_flag", C.c_uint64), ("skipped_mapq", C.c_uint64), ("unplaced", C.c_uint64),
                ("clipped", C.c_uint64), ("blocks", C.c_uint64), ("bad_records", C.c_uint64), ("first_bad_record", C.c_uint64),
                ("bad_reason", C.c_uint32), ("pad", C.c_uint32), ("t_add", C.c_double), ("t_total", C.c_double)]


# moni_cov_ref_t: the figures of one reference of a sealed coverage object
COV_REF_DTYPE = np.dtype([("length", np.uint64), ("bases", np.uint64), ("min", np.uint32), ("max", np.uint32)])
COV_EXCLUDE_DEFAULT = 0x704
assert COV_REF_DTYPE.itemsize == 24 and C.sizeof(CovStatsC) == 96


def bam_merge_plan(keys, offs, chunk_bytes: int) -> np.ndarray:
    """moni_bam_merge_plan (host only): runs r with keys[r] (ascending uint64) and offs[r] (len(keys[r]) + 1 offsets) -> cuts[n_chunks + 1, n_runs]:
    chunk k takes records cuts[k, r] .. cuts[k + 1, r] of run r."""
    L = lib()
    R = len(keys)
    ks = [np.ascontiguousarray(k, dtype=np.uint64) for k in keys]
    os_ = [np.ascontiguousarray(o, dtype=np.uint64) for o in offs]
    if any(len(o) != len(k) + 1 for k, o in zip(ks, os_)) or len(os_) != R:
        raise ValueError("bam_merge_plan: a run's offsets are one more than its keys")
    kp = (C.c_void_p * max(R, 1))(*[k.ctypes.data for k in ks])
    op = (C.c_void_p * max(R, 1))(*[o.ctypes.data for o in os_])
    n = np.array([len(k) for k in ks], dtype=np.uint64)
    plan = C.POINTER(BamPlanC)()
    _chk(L.moni_bam_merge_plan(kp, n.ctypes.data if R else None, op, R, chunk_bytes, C.byref(plan)), "moni_bam_merge_plan")
    try:
        nc = int(plan.contents.n_chunks)
        return np.ctypeslib.as_array(plan.contents.cuts, shape=((nc + 1) * R,)).reshape(nc + 1, R).copy() if R else np.zeros((1, 0), np.uint64)
    finally:
        L.moni_bam_plan_free(plan)


class BaiBuilder:
    """moni_bai_* (host only): the .bai of a coordinate-sorted BAM written as chunks of BGZF blocks, fed in file order"""

    def __init__(self, n_ref: int):
        self._L = lib()
        self._h = self._L.moni_bai_create(n_ref)
        if not self._h:
            raise MemoryError("moni_bai_create")

    def add(self, ents, chunk_len: int, block_size: int, csizes, file_off: int):
        e = np.ascontiguousarray(ents, dtype=BAM_ENT_DTYPE)
        cs = np.ascontiguousarray(csizes, dtype=np.uint32)
        _chk(self._L.moni_bai_add(self._h, e.ctypes.data if e.size else None, e.size, chunk_len, block_size, cs.ctypes.data if cs.size else None, cs.size,
                                  file_off), "moni_bai_add")

    def finish(self, eof_off: int) -> bytes:
        out, n = C.c_void_p(), C.c_uint64()
        _chk(self._L.moni_bai_finish(self._h, eof_off, C.byref(out), C.byref(n)), "moni_bai_finish")
        return C.string_at(out.value, n.value)

    def close(self):
        if self._h:
            self._L.moni_bai_destroy(self._h)
            self._h = None

    __del__ = close


class DpParamsC(C.Structure):
    _fields_ = [("m", C.c_int8), ("mat", C.c_int8 * 25), ("q", C.c_int8), ("e", C.c_int8),
                ("w", C.c_int32), ("zdrop", C.c_int32), ("end_bonus", C.c_int32)]


MEM_DTYPE = np.dtype([("pos", "<u8"), ("len", "<u4"), ("idx", "<u4"), ("rpos", "<u4"), ("mate", "<u4"),
                      ("total_occ", "<u4"), ("num_filtered", "<u4"), ("occ_off", "<u8"), ("occ_cnt", "<u4"),
                      ("read", "<u4")])
DP_TASK_DTYPE = np.dtype([("q_off", "<u8"), ("t_off", "<u8"), ("qlen", "<i4"), ("tlen", "<i4"), ("flag", "<i4"),
                          ("reserved", "<i4")])
DP_RESULT_DTYPE = np.dtype([("max", "<i4"), ("max_q", "<i4"), ("max_t", "<i4"), ("mqe", "<i4"), ("mqe_t", "<i4"),
                            ("mte", "<i4"), ("mte_q", "<i4"), ("score", "<i4"), ("reach_end", "<i4"),
                            ("zdropped", "<i4"), ("n_cigar", "<u4"), ("cigar_off", "<u4")])
LOCATE_RES_DTYPE = np.dtype([("count", "<u8"), ("sa_lo", "<u8"), ("occ_off", "<u8"), ("n_occ", "<u4"), ("matched", "<u4")])
SEQCOUNT_RES_DTYPE = np.dtype([("count", "<u8"), ("sa_lo", "<u8"), ("matched", "<u4"), ("n_seqs", "<u4"), ("walked", "<u4"), ("n_segs", "<u4")])
LOCI_RES_DTYPE = np.dtype([("count", "<u8"), ("sa_lo", "<u8"), ("loci_off", "<u8"), ("n_loci", "<u8"), ("matched", "<u4"), ("walked", "<u4"), ("n_segs", "<u4"),
                           ("reserved", "<u4")])
APPROX_RES_DTYPE = np.dtype([("cnt", "<u8", (4,)), ("n_hits", "<u8"), ("hit_off", "<u8"), ("n_kept", "<u4"), ("complete", "<u4"), ("matched", "<u4"), ("reserved", "<u4")])
APPROX_HIT_DTYPE = np.dtype([("task", "<u8"), ("n_mis", "<u4"), ("n_occ", "<u4"), ("sa_lo", "<u8"), ("count", "<u8"), ("occ_off", "<u8")])
APPROX_MAX_STEPS_DEFAULT = 1 << 20
APPROX_CHUNK_LEN_DEFAULT = 1 << 30
assert LOCATE_RES_DTYPE.itemsize == 32 and SEQCOUNT_RES_DTYPE.itemsize == 32 and APPROX_RES_DTYPE.itemsize == 64 and APPROX_HIT_DTYPE.itemsize == 40
assert LOCI_RES_DTYPE.itemsize == 48
SCREEN_RES_DTYPE = np.dtype([("n_win", "<u4"), ("n_pos", "<u4", (2,)), ("d_max", "<u4", (2,)), ("max_pml", "<u4", (2,)), ("flags", "<u4")])
SCREEN_BINS, SCREEN_PRESENT, SCREEN_STRAND1, SCREEN_SHORT = 32, 1, 2, 4
assert SCREEN_RES_DTYPE.itemsize == 32 and C.sizeof(ScreenParamsC) == 32
assert MEM_DTYPE.itemsize == 48 and DP_TASK_DTYPE.itemsize == 32 and DP_RESULT_DTYPE.itemsize == 48

DEFAULT_MAT = [2, -4, -4, -4, 0, -4, 2, -4, -4, 0, -4, -4, 2, -4, 0, -4, -4, -4, 2, 0, 0, 0, 0, 0, 0]

_lib = None


def build_lib(force: bool = False) -> str:
    """hipcc cross-compiles for gfx950 without a GPU."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".hpp", ".inc", ".cpp"))]
    srcs.append(os.path.join(os.path.dirname(HERE), "include", "moni_hip.h"))
    if force or not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs):
        # pe_big.cpp: host-only translation unit (the paired state machine with large capacities, its own namespace)
        big_o = os.path.join(CSRC, "pe_big.o")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-c", os.path.join(CSRC, "pe_big.cpp"), "-o", big_o])
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                               "-o", LIB_PATH, os.path.join(CSRC, "moni_hip.hip"), "-Wl," + big_o])      # (as a linker input: hipcc would read a bare .o as HIP source)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libmoni_hip.so is not built (run __graft_entry__.build()); there is no fallback path")
        L = C.CDLL(LIB_PATH)
        L.moni_version.restype = C.c_char_p
        L.moni_index_n.restype = C.c_uint64
        L.moni_index_r.restype = C.c_uint64
        L.moni_index_device_bytes.restype = C.c_uint64
        for name in ("moni_index_n", "moni_index_r", "moni_index_device_bytes", "moni_index_destroy",
                     "moni_ctx_destroy", "moni_free"):
            getattr(L, name).argtypes = [C.c_void_p]
        L.moni_index_text.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.moni_index_create.argtypes = [C.POINTER(FlatIndexC), C.c_int, C.POINTER(C.c_void_p)]
        L.moni_index_load.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
        L.moni_ctx_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.moni_reads_upload.argtypes = [C.c_void_p, C.POINTER(ReadBatchC)]
        L.moni_reads_swap.argtypes = [C.c_void_p, C.c_uint32]
        L.moni_ms_run.argtypes = [C.c_void_p]
        L.moni_ms_query_batch.argtypes = [C.c_void_p, C.POINTER(ReadBatchC), C.c_void_p]
        L.moni_seed_run.argtypes = [C.c_void_p, C.POINTER(SeedParamsC)]
        L.moni_seed_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.moni_seed_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.moni_phi_lcp_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
        L.moni_extz_batch.argtypes = [C.c_void_p, C.POINTER(DpParamsC), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                      C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.moni_align_params_default.argtypes = [C.POINTER(AlignParamsC)]
        L.moni_align_params_default.restype = None
        L.moni_align_batch.argtypes = [C.c_void_p, C.POINTER(ReadBatchC), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(AlignParamsC),
                                       C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(AlignStatsC)]
        L.moni_align_stream.argtypes = L.moni_align_batch.argtypes
        L.moni_align_csv_batch.argtypes = [C.c_void_p, C.POINTER(ReadBatchC), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(AlignParamsC),
                                           C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(AlignStatsC)]
        L.moni_pe_params_default.argtypes = [C.POINTER(PeParamsC)]
        L.moni_pe_params_default.restype = None
        L.moni_pe_learn_batch.argtypes = [C.c_void_p, C.POINTER(ReadBatchC), C.POINTER(AlignParamsC), C.POINTER(PeParamsC), C.POINTER(PeModelC)]
        L.moni_pe_align_batch.argtypes = [C.c_void_p, C.POINTER(ReadBatchC), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(AlignParamsC),
                                          C.POINTER(PeParamsC), C.POINTER(PeModelC), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(AlignStatsC)]
        L.moni_pe_align_stream.argtypes = L.moni_pe_align_batch.argtypes
        L.moni_pe_align_csv_batch.argtypes = L.moni_pe_align_batch.argtypes[:-1] + [C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(AlignStatsC)]
        L.moni_pe_align_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(AlignParamsC), C.POINTER(PeParamsC), C.POINTER(PeModelC),
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(AlignStatsC)]
        L.moni_pe_report_mems_batch.argtypes = [C.c_void_p, C.POINTER(ReadBatchC), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(AlignParamsC), C.POINTER(PeParamsC),
                                                C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.moni_align_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(AlignParamsC),
                                     C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(AlignStatsC)]
        L.moni_extend_params_default.argtypes = [C.POINTER(ExtendParamsC)]
        L.moni_extend_params_default.restype = None
        L.moni_extend_batch.argtypes = [C.c_void_p, C.POINTER(ReadBatchC), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ExtendParamsC),
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(ExtendStatsC)]
        L.moni_extend_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ExtendParamsC),
                                      C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(ExtendStatsC)]
        L.moni_pml_batch.argtypes = [C.c_void_p, C.POINTER(ReadBatchC), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.moni_pml_run.argtypes = [C.c_void_p, C.c_uint32]
        L.moni_pml_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.moni_pml_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.moni_screen_params_default.argtypes = [C.POINTER(ScreenParamsC)]
        L.moni_screen_params_default.restype = None
        L.moni_screen_run.argtypes = [C.c_void_p, C.POINTER(ScreenParamsC)]
        L.moni_screen_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.moni_screen_fetch.argtypes = [C.c_void_p, C.c_void_p]
        L.moni_screen_batch.argtypes = [C.c_void_p, C.POINTER(ReadBatchC), C.POINTER(ScreenParamsC), C.c_void_p]
        L.moni_locate_params_default.argtypes = [C.POINTER(LocateParamsC)]
        L.moni_locate_params_default.restype = None
        L.moni_locate_run.argtypes = [C.c_void_p, C.POINTER(LocateParamsC)]
        L.moni_locate_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.moni_locate_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.moni_seqcount_params_default.argtypes = [C.POINTER(SeqcountParamsC)]
        L.moni_seqcount_params_default.restype = None
        L.moni_seqcount_run.argtypes = [C.c_void_p, C.POINTER(SeqcountParamsC)]
        L.moni_seqcount_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        L.moni_seqcount_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.moni_seqcount_batch.argtypes = [C.c_void_p, C.POINTER(ReadBatchC), C.POINTER(SeqcountParamsC), C.c_void_p, C.c_void_p]
        L.moni_loci_params_default.argtypes = [C.POINTER(LociParamsC)]
        L.moni_loci_params_default.restype = None
        L.moni_loci_run.argtypes = [C.c_void_p, C.POINTER(LociParamsC)]
        L.moni_loci_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.moni_loci_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.moni_loci_batch.argtypes = [C.c_void_p, C.POINTER(ReadBatchC), C.POINTER(LociParamsC), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                      C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.moni_approx_params_default.argtypes = [C.POINTER(ApproxParamsC)]
        L.moni_approx_params_default.restype = None
        L.moni_approx_run.argtypes = [C.c_void_p, C.POINTER(ApproxParamsC)]
        L.moni_approx_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.moni_approx_fetch.argtypes = [C.c_void_p] + [C.c_void_p] * 5
        L.moni_approx_batch.argtypes = [C.c_void_p, C.POINTER(ReadBatchC), C.POINTER(ApproxParamsC), C.c_void_p] + [C.POINTER(C.c_void_p)] * 4 + [C.POINTER(C.c_uint64)] * 2
        L.moni_locate_batch.argtypes = [C.c_void_p, C.POINTER(ReadBatchC), C.POINTER(LocateParamsC), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.moni_sam_header.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.moni_last_kernel_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float)]
        L.moni_last_counters.argtypes = [C.c_void_p, C.c_void_p]
        L.moni_seed_occ_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.moni_seed_prefilter.argtypes = [C.c_void_p, C.c_int]
        L.moni_seed_prefilter_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.moni_ms_leap_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.moni_index_leap_table.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
        L.moni_ms_lengths_batch.argtypes = [C.c_void_p, C.POINTER(ReadBatchC), C.c_void_p, C.c_void_p]
        L.moni_mslong_params_default.argtypes = [C.POINTER(MslongParamsC)]
        L.moni_mslong_params_default.restype = None
        L.moni_ms_long_batch.argtypes = [C.c_void_p, C.POINTER(ReadBatchC), C.POINTER(MslongParamsC), C.c_void_p, C.c_void_p, C.POINTER(MslongStatsC)]
        L.moni_report_mems_batch.argtypes = [C.c_void_p, C.POINTER(ReadBatchC), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(AlignParamsC),
                                             C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.moni_ldx_info.argtypes = [C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        L.moni_ldx_rewrite.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
        L.moni_ldx_write.argtypes = [C.POINTER(FlatIndexC), C.c_char_p, C.c_int]
        L.moni_ms_file_info.argtypes = [C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.moni_ms_file_read.argtypes = [C.c_char_p, C.c_uint64] + [C.c_void_p] * 7 + [C.c_char_p, C.c_uint64]
        L.moni_ms_file_write.argtypes = [C.POINTER(FlatIndexC), C.c_char_p]
        L.moni_index_load_reference.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
        L.moni_ldx_lift_batch.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
        L.moni_bgzf_params_default.argtypes = [C.POINTER(BgzfParamsC)]
        L.moni_bgzf_params_default.restype = None
        L.moni_bgzf_compress.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(BgzfParamsC), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                         C.POINTER(BgzfStatsC)]
        L.moni_bam_params_default.argtypes = [C.POINTER(BamParamsC)]
        L.moni_bam_params_default.restype = None
        L.moni_bam_set_header.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.moni_bam_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(BamParamsC), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                       C.POINTER(BamStatsC)]
        L.moni_bam_sorted_run.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(BamSortStatsC)]
        L.moni_bam_sort.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(BamParamsC), C.POINTER(C.c_void_p),
                                    C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(BamSortStatsC)]
        L.moni_bam_sorted_run_dup.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p),
                                              C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(BamRunDupStatsC)]
        L.moni_bam_dup_resolve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(BamDupStatsC)]
        L.moni_bam_sort_marked.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(BamParamsC), C.POINTER(C.c_void_p),
                                           C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(BamSortStatsC)]
        L.moni_bam_merge_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.POINTER(BamPlanC))]
        L.moni_bam_plan_free.argtypes = [C.POINTER(BamPlanC)]
        L.moni_bam_plan_free.restype = None
        L.moni_bai_create.argtypes = [C.c_uint32]
        L.moni_bai_create.restype = C.c_void_p
        L.moni_bai_add.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64]
        L.moni_bai_finish.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.moni_bai_destroy.argtypes = [C.c_void_p]
        L.moni_bai_destroy.restype = None
        L.moni_inflate_params_default.argtypes = [C.POINTER(InflateParamsC)]
        L.moni_inflate_params_default.restype = None
        L.moni_bgzf_scan.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.moni_bgzf_inflate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(InflateParamsC), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                        C.POINTER(InflateStatsC)]
        L.moni_bamin_params_default.argtypes = [C.POINTER(BamInParamsC)]
        L.moni_bamin_params_default.restype = None
        L.moni_bam_in_reset.argtypes = [C.c_void_p]
        L.moni_bam_in_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(BamInParamsC), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(BamInStatsC)]
        L.moni_cov_params_default.argtypes = [C.POINTER(CovParamsC)]
        L.moni_cov_params_default.restype = None
        L.moni_cov_create.argtypes = [C.c_void_p, C.POINTER(CovParamsC), C.POINTER(C.c_void_p)]
        L.moni_cov_destroy.argtypes = [C.c_void_p]
        L.moni_cov_destroy.restype = None
        L.moni_cov_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(CovStatsC)]
        L.moni_cov_add_sorted.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(CovStatsC)]
        L.moni_cov_seal.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
        L.moni_cov_next.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        L.moni_cov_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.moni_cov_test_set_counted.argtypes = [C.c_void_p, C.c_uint64]
        L.moni_cov_test_set_counted.restype = None
        _lib = L
    return _lib


HANDOVER_WHY = ("long_read", "anchors", "chains", "chains_to_score", "chain_anchors", "dp_size", "unused", "wildcard_or_dirs", "loop_depends_on_score",
                "extension_short_of_end", "capacity", "cigar_md_line")


def _stats_dict(st) -> dict:
    d = {k: getattr(st, k) for k, _ in AlignStatsC._fields_ if k != "handover_why"}
    d["handover_why"] = {HANDOVER_WHY[i]: int(st.handover_why[i]) for i in range(12) if st.handover_why[i]}
    return d


def _chk(rc: int, what: str):
    if rc != 0:
        raise RuntimeError("%s failed with code %d" % (what, rc))


def flat_struct(fi, without_text: bool = False, without_lcp: bool = False) -> FlatIndexC:
    """fi: moni_align_amd.index_build.FlatIndex (arrays are kept alive by the caller).  without_text: text = NULL (rebuilt from the BWT);
    without_lcp: slcp = NULL (the `-n` form: <prefix>.thrbv.full.ms)."""
    s = FlatIndexC()
    s.n, s.r, s.w, s.n_seq = fi.n, fi.r, fi.w, len(fi.seq_starts) - 1
    for k in ("F", "heads", "starts", "ssa", "esa", "thr", "seq_starts") + (() if without_text else ("text",)) + (() if without_lcp else ("slcp",)):
        a = getattr(fi, k)
        assert a.flags["C_CONTIGUOUS"]
        setattr(s, k, a.ctypes.data)
    s._names_keep = b"".join(x.encode() + b"\0" for x in fi.names)
    s.seq_names = s._names_keep
    lf = getattr(fi, "lifts", None)
    if lf is not None:           # VCF-built index: one lift per sequence (liftidx.hpp:131-143); absent = null lifts
        s.lift_second, s.lift_len = lf.second.ctypes.data, lf.len.ctypes.data
        s.lift_ins_off, s.lift_ins = lf.ins_off.ctypes.data, lf.ins.ctypes.data
        s.lift_del_off, s.lift_del = lf.del_off.ctypes.data, lf.dele.ctypes.data
    return s


class Coverage:
    """moni_cov_*: the depth of coverage of the records added, over the dictionary of the header set on `ctx`.  Every method
    takes the context it runs on; an add may run on any context of the same device, from several threads at once.  The calls return the
    library's code first, so that a test sees a refusal as it is; rc_only=False raises on any code but 0."""

    def __init__(self, ctx, exclude_flags: int = COV_EXCLUDE_DEFAULT, min_mapq: int = 0, reserved=(0, 0)):
        self._L = lib()
        self._h = C.c_void_p()
        p = CovParamsC()
        self._L.moni_cov_params_default(C.byref(p))
        assert p.exclude_flags == COV_EXCLUDE_DEFAULT and p.min_mapq == 0
        p.exclude_flags, p.min_mapq = exclude_flags, min_mapq
        p.reserved[0], p.reserved[1] = reserved
        self.rc = self._L.moni_cov_create(ctx._h, C.byref(p), C.byref(self._h))
        if self.rc:
            self._h = C.c_void_p()
            raise ValueError("moni_cov_create failed with code %d" % self.rc)

    @staticmethod
    def _stats(st):
        return {k: getattr(st, k) for k, _ in CovStatsC._fields_ if k != "pad"}

    def add(self, ctx, records, offs):
        """moni_cov_add: (rc, stats)"""
        buf = np.frombuffer(records, dtype=np.uint8) if isinstance(records, (bytes, bytearray, memoryview)) else np.ascontiguousarray(records, dtype=np.uint8)
        o = np.ascontiguousarray(offs, dtype=np.uint64)
        st = CovStatsC()
        rc = self._L.moni_cov_add(ctx._h, self._h, buf.ctypes.data if buf.size else None, buf.size, o.ctypes.data if o.size else None, max(len(o) - 1, 0), C.byref(st))
        return rc, self._stats(st)

    def add_sorted(self, ctx):
        """moni_cov_add_sorted: (rc, stats)"""
        st = CovStatsC()
        rc = self._L.moni_cov_add_sorted(ctx._h, self._h, C.byref(st))
        return rc, self._stats(st)

    def seal(self, ctx):
        """moni_cov_seal: (rc, [(length, bases, min, max)] per reference)"""
        refs, n = C.c_void_p(), C.c_uint32()
        rc = self._L.moni_cov_seal(ctx._h, self._h, C.byref(refs), C.byref(n))
        if rc or not n.value:
            return rc, []
        a = np.frombuffer(C.string_at(refs.value, COV_REF_DTYPE.itemsize * n.value), dtype=COV_REF_DTYPE)
        return rc, [tuple(int(x) for x in r) for r in a]

    def next(self, ctx, max_bases: int, max_lines: int):
        """moni_cov_next: (rc, the piece of text, done)"""
        t, n, done = C.c_void_p(), C.c_uint64(), C.c_int()
        rc = self._L.moni_cov_next(ctx._h, self._h, max_bases, max_lines, C.byref(t), C.byref(n), C.byref(done))
        return rc, (C.string_at(t.value, n.value) if rc == 0 and n.value else b""), done.value

    def text(self, ctx, max_bases: int = 1 << 26, max_lines: int = 1 << 22) -> bytes:
        """the whole per-base text: the pieces of moni_cov_next until done"""
        out = []
        while True:
            rc, piece, done = self.next(ctx, max_bases, max_lines)
            _chk(rc, "moni_cov_next")
            out.append(piece)
            if done:
                return b"".join(out)

    def windows(self, ctx, ref_id: int, window: int):
        """moni_cov_windows: (rc, [sum of the depth per window])"""
        p, n = C.c_void_p(), C.c_uint64()
        rc = self._L.moni_cov_windows(ctx._h, self._h, ref_id, window, C.byref(p), C.byref(n))
        return rc, (np.frombuffer(C.string_at(p.value, 8 * n.value), dtype=np.uint64).tolist() if rc == 0 and n.value else [])

    def test_set_counted(self, counted: int):
        self._L.moni_cov_test_set_counted(self._h, counted)

    def close(self):
        if self._h:
            self._L.moni_cov_destroy(self._h)
            self._h = C.c_void_p()


class Index:
    def __init__(self, fi=None, path: Optional[str] = None, device: int = 0, reference=None, without_text: bool = False, without_lcp: bool = False):
        """fi: a FlatIndex; path: an .mfi file; reference: (<prefix>.thrbv.full.lcp.ms, <prefix>.ldx, text file) of the reference."""
        self._L = lib()
        self._h = C.c_void_p()
        self._keep = fi
        if reference is not None:
            ms, ldx, text = reference
            _chk(self._L.moni_index_load_reference(ms.encode(), ldx.encode(), text.encode() if text else None, device, C.byref(self._h)), "moni_index_load_reference")
        elif fi is not None:
            st = flat_struct(fi, without_text, without_lcp)
            _chk(self._L.moni_index_create(C.byref(st), device, C.byref(self._h)), "moni_index_create")
        else:
            _chk(self._L.moni_index_load(path.encode(), device, C.byref(self._h)), "moni_index_load")
        self.n = self._L.moni_index_n(self._h)
        self.r = self._L.moni_index_r(self._h)
        self.device_bytes = self._L.moni_index_device_bytes(self._h)

    def leap_table(self, fetch: bool = True):
        """the sampled inverse suffix array of the leaping walk (moni_index_leap_table): stride, build time in ms, and with fetch the entries
        (run | off << 32) and their clean bytes; stride 0 and empty arrays for an index made under MONI_MS_LEAP=0"""
        n_ent, stride, ms = C.c_uint64(), C.c_uint32(), C.c_float()
        _chk(self._L.moni_index_leap_table(self._h, None, None, 0, C.byref(n_ent), C.byref(stride), C.byref(ms)), "moni_index_leap_table")
        isa = np.zeros(n_ent.value if fetch else 0, dtype=np.uint64)
        clean = np.zeros(n_ent.value if fetch else 0, dtype=np.uint8)
        if fetch and n_ent.value:
            _chk(self._L.moni_index_leap_table(self._h, isa.ctypes.data, clean.ctypes.data, n_ent.value, None, None, None), "moni_index_leap_table")
        return {"stride": int(stride.value), "build_ms": float(ms.value), "isa": isa, "clean": clean}

    def text(self) -> np.ndarray:
        """the text of the index (n - 1 bytes), as handed over or as rebuilt from the BWT"""
        out = np.empty(self.n - 1, dtype=np.uint8)
        _chk(self._L.moni_index_text(self._h, out.ctypes.data, out.size), "moni_index_text")
        return out

    def close(self):
        if self._h:
            self._L.moni_index_destroy(self._h)
            self._h = C.c_void_p()


class Ctx:
    def __init__(self, index: Index):
        self._L = lib()
        self.index = index
        self._h = C.c_void_p()
        _chk(self._L.moni_ctx_create(index._h, C.byref(self._h)), "moni_ctx_create")
        self.n_reads = 0
        self._parked = {}

    def close(self):
        if self._h:
            self._L.moni_ctx_destroy(self._h)
            self._h = C.c_void_p()

    @staticmethod
    def _batch(seq: np.ndarray, offsets: np.ndarray):
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        b = ReadBatchC(seq.ctypes.data, offsets.ctypes.data, len(offsets) - 1)
        return b, (seq, offsets)

    def upload(self, seq: np.ndarray, offsets: np.ndarray):
        b, keep = self._batch(seq, offsets)
        _chk(self._L.moni_reads_upload(self._h, C.byref(b)), "moni_reads_upload")
        self.n_reads = len(offsets) - 1

    def swap(self, slot: int):
        """exchange the resident batch with the one parked in `slot` (moni_reads_swap)"""
        _chk(self._L.moni_reads_swap(self._h, slot), "moni_reads_swap")
        self.n_reads, self._parked[slot] = self._parked.get(slot, 0), self.n_reads

    def ms_run(self):
        _chk(self._L.moni_ms_run(self._h), "moni_ms_run")

    def ms_query_batch(self, seq: np.ndarray, offsets: np.ndarray) -> np.ndarray:
        b, keep = self._batch(seq, offsets)
        total = int(keep[1][-1] - keep[1][0])
        out = np.empty(2 * total, dtype=np.uint64)
        _chk(self._L.moni_ms_query_batch(self._h, C.byref(b), out.ctypes.data), "moni_ms_query_batch")
        self.n_reads = len(offsets) - 1
        return out

    def seed_run(self, min_len: int = 25, filter_seeds: bool = True, n_seeds_thr: int = 1000, report_mems: bool = False):
        p = SeedParamsC(min_len, int(filter_seeds), n_seeds_thr, int(report_mems))
        _chk(self._L.moni_seed_run(self._h, C.byref(p)), "moni_seed_run")

    def seed_fetch(self) -> Dict[str, np.ndarray]:
        nm, no = C.c_uint64(), C.c_uint64()
        _chk(self._L.moni_seed_counts(self._h, C.byref(nm), C.byref(no)), "moni_seed_counts")
        mems = np.empty(nm.value, dtype=MEM_DTYPE)
        occs = np.empty(no.value, dtype=np.uint64)
        rmo = np.empty(self.n_reads + 1, dtype=np.uint64)
        _chk(self._L.moni_seed_fetch(self._h, mems.ctypes.data, occs.ctypes.data, rmo.ctypes.data), "moni_seed_fetch")
        return {"mems": mems, "occs": occs, "read_mem_off": rmo}

    def phi_lcp_batch(self, pos: np.ndarray, inverse: bool = False):
        pos = np.ascontiguousarray(pos, dtype=np.uint64)
        a = np.empty(len(pos), dtype=np.uint64)
        b = np.empty(len(pos), dtype=np.uint64)
        _chk(self._L.moni_phi_lcp_batch(self._h, pos.ctypes.data, len(pos), int(inverse), a.ctypes.data, b.ctypes.data),
             "moni_phi_lcp_batch")
        return a, b

    def extz_batch(self, qseq: np.ndarray, tseq: np.ndarray, tasks: np.ndarray, cigar_cap: Optional[int] = None,
                   mat=DEFAULT_MAT, q: int = 4, e: int = 2, w: int = -1, zdrop: int = -1, end_bonus: int = 400):
        qseq = np.ascontiguousarray(qseq, dtype=np.uint8)
        tseq = np.ascontiguousarray(tseq, dtype=np.uint8)
        tasks = np.ascontiguousarray(tasks, dtype=DP_TASK_DTYPE)
        prm = DpParamsC()
        prm.m = 5
        for i, v in enumerate(mat):
            prm.mat[i] = v
        prm.q, prm.e, prm.w, prm.zdrop, prm.end_bonus = q, e, w, zdrop, end_bonus
        res = np.zeros(len(tasks), dtype=DP_RESULT_DTYPE)
        if cigar_cap is None:
            cigar_cap = int((tasks["qlen"].astype(np.int64) + tasks["tlen"].astype(np.int64)).sum()) + 16
        pool = np.zeros(cigar_cap, dtype=np.uint32)
        used = C.c_uint64()
        _chk(self._L.moni_extz_batch(self._h, C.byref(prm), qseq.ctypes.data, len(qseq), tseq.ctypes.data, len(tseq),
                                     tasks.ctypes.data, len(tasks), res.ctypes.data, pool.ctypes.data, cigar_cap,
                                     C.byref(used)), "moni_extz_batch")
        return res, pool[: used.value]

    def align_batch(self, seq: np.ndarray, offsets: np.ndarray, names: np.ndarray, name_off: np.ndarray, quals=None,
                    host_threads: Optional[int] = None, stream: bool = False, want_text: bool = True, **overrides):
        """SAM text (bytes) of the batch + stats dict; the whole single-end path on the GPU + host stages.
        stream=True: moni_align_stream (text in the context-owned pinned buffer, lines ordered on the GPU); want_text=False
        (with stream) returns the text's length instead of copying it into a Python bytes object."""
        b, keep = self._batch(seq, offsets)
        names = np.ascontiguousarray(names, dtype=np.uint8)
        name_off = np.ascontiguousarray(name_off, dtype=np.uint64)
        if quals is not None:
            quals = np.ascontiguousarray(quals, dtype=np.uint8)
        prm = AlignParamsC()
        self._L.moni_align_params_default(C.byref(prm))
        if host_threads is not None:
            prm.host_threads = host_threads
        for k, v in overrides.items():
            setattr(prm, k, v)
        out = C.c_void_p()
        ln = C.c_uint64()
        st = AlignStatsC()
        fn = self._L.moni_align_stream if stream else self._L.moni_align_batch
        _chk(fn(self._h, C.byref(b), names.ctypes.data, name_off.ctypes.data,
                quals.ctypes.data if quals is not None else None, C.byref(prm), C.byref(out), C.byref(ln),
                C.byref(st)), "moni_align_stream" if stream else "moni_align_batch")
        self.n_reads = len(offsets) - 1
        try:
            sam = C.string_at(out, ln.value) if (want_text or not stream) else int(ln.value)
        finally:
            if not stream:
                self._L.moni_free(out)
        return sam, _stats_dict(st)

    def align_csv_batch(self, seq, offsets, names, name_off, quals=None, host_threads: Optional[int] = None, **overrides):
        """(SAM text, CSV lines, stats) of moni_align_csv_batch (`-c`)"""
        b, keep = self._batch(seq, offsets)
        names = np.ascontiguousarray(names, dtype=np.uint8)
        name_off = np.ascontiguousarray(name_off, dtype=np.uint64)
        if quals is not None:
            quals = np.ascontiguousarray(quals, dtype=np.uint8)
        prm = AlignParamsC()
        self._L.moni_align_params_default(C.byref(prm))
        if host_threads is not None:
            prm.host_threads = host_threads
        for k, v in overrides.items():
            setattr(prm, k, v)
        sam, sl, csv, cl = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
        st = AlignStatsC()
        _chk(self._L.moni_align_csv_batch(self._h, C.byref(b), names.ctypes.data, name_off.ctypes.data, quals.ctypes.data if quals is not None else None, C.byref(prm),
                                          C.byref(sam), C.byref(sl), C.byref(csv), C.byref(cl), C.byref(st)), "moni_align_csv_batch")
        self.n_reads = len(offsets) - 1
        try:
            return C.string_at(sam, sl.value), C.string_at(csv, cl.value), _stats_dict(st)
        finally:
            self._L.moni_free(sam); self._L.moni_free(csv)

    def _pe_params(self, host_threads, overrides):
        prm = AlignParamsC()
        self._L.moni_align_params_default(C.byref(prm))
        if host_threads is not None:
            prm.host_threads = host_threads
        pe = PeParamsC()
        self._L.moni_pe_params_default(C.byref(pe))
        for k, v in overrides.items():
            setattr(pe if hasattr(pe, k) and not hasattr(prm, k) else prm, k, v)
        return prm, pe

    def pe_learn(self, seq: np.ndarray, offsets: np.ndarray, model: Optional["PeModelC"] = None, **overrides):
        """learn_fragment_model over one batch of interleaved pairs (reads 2p, 2p+1); returns the updated model."""
        b, keep = self._batch(seq, offsets)
        prm, pe = self._pe_params(None, overrides)
        model = model if model is not None else PeModelC()
        _chk(self._L.moni_pe_learn_batch(self._h, C.byref(b), C.byref(prm), C.byref(pe), C.byref(model)), "moni_pe_learn_batch")
        return model

    def pe_align(self, seq: np.ndarray, offsets: np.ndarray, names: np.ndarray, name_off: np.ndarray, quals, model: "PeModelC",
                 host_threads: Optional[int] = None, want_text: bool = True, stream: bool = False, **overrides):
        """SAM text (bytes) of the interleaved pairs + stats dict (moni_pe_align_batch; stream=True: moni_pe_align_stream, the text in the
        context-owned buffer); want_text=False returns the text's length instead of copying it into a Python bytes object (the library has
        still produced the text in host memory)."""
        b, keep = self._batch(seq, offsets)
        names = np.ascontiguousarray(names, dtype=np.uint8)
        name_off = np.ascontiguousarray(name_off, dtype=np.uint64)
        if quals is not None:
            quals = np.ascontiguousarray(quals, dtype=np.uint8)
        prm, pe = self._pe_params(host_threads, overrides)
        out = C.c_void_p()
        ln = C.c_uint64()
        st = AlignStatsC()
        fn = self._L.moni_pe_align_stream if stream else self._L.moni_pe_align_batch
        _chk(fn(self._h, C.byref(b), names.ctypes.data, name_off.ctypes.data, quals.ctypes.data if quals is not None else None,
                C.byref(prm), C.byref(pe), C.byref(model), C.byref(out), C.byref(ln), C.byref(st)), "moni_pe_align_stream" if stream else "moni_pe_align_batch")
        try:
            sam = C.string_at(out, ln.value) if want_text else int(ln.value)
        finally:
            if not stream:
                self._L.moni_free(out)
        return sam, _stats_dict(st)

    def pe_align_csv(self, seq, offsets, names, name_off, quals, model: "PeModelC", host_threads: Optional[int] = None, **overrides):
        """(SAM text, CSV lines, stats) of moni_pe_align_csv_batch (`-c` for pairs: one line per pair)"""
        b, keep = self._batch(seq, offsets)
        names = np.ascontiguousarray(names, dtype=np.uint8)
        name_off = np.ascontiguousarray(name_off, dtype=np.uint64)
        if quals is not None:
            quals = np.ascontiguousarray(quals, dtype=np.uint8)
        prm, pe = self._pe_params(host_threads, overrides)
        sam, sl, csv, cl, st = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64(), AlignStatsC()
        _chk(self._L.moni_pe_align_csv_batch(self._h, C.byref(b), names.ctypes.data, name_off.ctypes.data, quals.ctypes.data if quals is not None else None,
                                             C.byref(prm), C.byref(pe), C.byref(model), C.byref(sam), C.byref(sl), C.byref(csv), C.byref(cl), C.byref(st)), "moni_pe_align_csv_batch")
        try:
            return C.string_at(sam, sl.value), C.string_at(csv, cl.value), _stats_dict(st)
        finally:
            self._L.moni_free(sam)
            self._L.moni_free(csv)

    def pe_align_run(self, names: np.ndarray, name_off: np.ndarray, quals, model: "PeModelC", host_threads: Optional[int] = None, want_text: bool = True, **overrides):
        """moni_pe_align_run over the interleaved pairs made resident by upload(); the text is in the context's buffer (want_text=False: its length)"""
        names = np.ascontiguousarray(names, dtype=np.uint8)
        name_off = np.ascontiguousarray(name_off, dtype=np.uint64)
        if quals is not None:
            quals = np.ascontiguousarray(quals, dtype=np.uint8)
        prm, pe = self._pe_params(host_threads, overrides)
        out, ln, st = C.c_void_p(), C.c_uint64(), AlignStatsC()
        _chk(self._L.moni_pe_align_run(self._h, names.ctypes.data, name_off.ctypes.data, quals.ctypes.data if quals is not None else None, C.byref(prm), C.byref(pe),
                                       C.byref(model), C.byref(out), C.byref(ln), C.byref(st)), "moni_pe_align_run")
        return (C.string_at(out, ln.value) if want_text else int(ln.value)), _stats_dict(st)

    def pe_report_mems(self, seq, offsets, names, name_off, quals=None, **overrides) -> bytes:
        """-m for pairs (moni_pe_report_mems_batch): the MEM records of the interleaved pairs"""
        b, keep = self._batch(seq, offsets)
        names = np.ascontiguousarray(names, dtype=np.uint8)
        name_off = np.ascontiguousarray(name_off, dtype=np.uint64)
        if quals is not None:
            quals = np.ascontiguousarray(quals, dtype=np.uint8)
        prm, pe = self._pe_params(None, overrides)
        out, ln = C.c_void_p(), C.c_uint64()
        _chk(self._L.moni_pe_report_mems_batch(self._h, C.byref(b), names.ctypes.data, name_off.ctypes.data, quals.ctypes.data if quals is not None else None,
                                               C.byref(prm), C.byref(pe), C.byref(out), C.byref(ln)), "moni_pe_report_mems_batch")
        self.n_reads = len(offsets) - 1
        try:
            return C.string_at(out, ln.value)
        finally:
            self._L.moni_free(out)

    def align_run(self, names: np.ndarray, name_off: np.ndarray, quals=None, host_threads: Optional[int] = None,
                  want_text: bool = True, **overrides):
        """moni_align_run over the batch made resident by upload(); want_text=False skips the copy into a Python bytes
        object (the library has still produced the SAM text) and returns its length instead."""
        names = np.ascontiguousarray(names, dtype=np.uint8)
        name_off = np.ascontiguousarray(name_off, dtype=np.uint64)
        if quals is not None:
            quals = np.ascontiguousarray(quals, dtype=np.uint8)
        prm = AlignParamsC()
        self._L.moni_align_params_default(C.byref(prm))
        if host_threads is not None:
            prm.host_threads = host_threads
        for k, v in overrides.items():
            setattr(prm, k, v)
        out = C.c_void_p()
        ln = C.c_uint64()
        st = AlignStatsC()
        _chk(self._L.moni_align_run(self._h, names.ctypes.data, name_off.ctypes.data, quals.ctypes.data if quals is not None else None,
                                    C.byref(prm), C.byref(out), C.byref(ln), C.byref(st)), "moni_align_run")
        sam = C.string_at(out, ln.value) if want_text else int(ln.value)      # the buffer belongs to the context
        return sam, _stats_dict(st)

    def _extend_params(self, overrides):
        prm = ExtendParamsC()
        self._L.moni_extend_params_default(C.byref(prm))
        for k, v in overrides.items():
            setattr(prm, k, v)
        return prm

    def extend_batch(self, seq: np.ndarray, offsets: np.ndarray, names: np.ndarray, name_off: np.ndarray, quals=None, **overrides):
        """moni_extend_batch (the legacy `moni extend`): (SAM records of the batch, no header; stats dict).  overrides: fields of
        moni_extend_params_t (min_len, ext_len, smatch, smismatch, gapo, gape, end_bonus)."""
        b, keep = self._batch(seq, offsets)
        names = np.ascontiguousarray(names, dtype=np.uint8)
        name_off = np.ascontiguousarray(name_off, dtype=np.uint64)
        if quals is not None:
            quals = np.ascontiguousarray(quals, dtype=np.uint8)
        prm = self._extend_params(overrides)
        out, ln, st = C.c_void_p(), C.c_uint64(), ExtendStatsC()
        _chk(self._L.moni_extend_batch(self._h, C.byref(b), names.ctypes.data, name_off.ctypes.data, quals.ctypes.data if quals is not None else None,
                                       C.byref(prm), C.byref(out), C.byref(ln), C.byref(st)), "moni_extend_batch")
        self.n_reads = len(offsets) - 1
        try:
            return C.string_at(out, ln.value), {f: getattr(st, f) for f, _ in ExtendStatsC._fields_}
        finally:
            self._L.moni_free(out)

    def extend_run(self, names: np.ndarray, name_off: np.ndarray, quals=None, want_text: bool = True, **overrides):
        """moni_extend_run over the batch made resident by upload(); want_text=False returns the length of the text instead of a copy."""
        names = np.ascontiguousarray(names, dtype=np.uint8)
        name_off = np.ascontiguousarray(name_off, dtype=np.uint64)
        if quals is not None:
            quals = np.ascontiguousarray(quals, dtype=np.uint8)
        prm = self._extend_params(overrides)
        out, ln, st = C.c_void_p(), C.c_uint64(), ExtendStatsC()
        _chk(self._L.moni_extend_run(self._h, names.ctypes.data, name_off.ctypes.data, quals.ctypes.data if quals is not None else None,
                                     C.byref(prm), C.byref(out), C.byref(ln), C.byref(st)), "moni_extend_run")
        sam = (C.string_at(out, ln.value) if ln.value else b"") if want_text else int(ln.value)      # the buffer belongs to the context
        return sam, {f: getattr(st, f) for f, _ in ExtendStatsC._fields_}

    def pml_batch(self, seq: np.ndarray, offsets: np.ndarray, thr: int = 25):
        """legacy `moni pseudo-ms` (moni_pml_batch): (lengths, read_max, read_hits) - the pseudo-matching length at every read offset (forward
        strand), the largest of each read, and the number of offsets of each read with a length >= thr"""
        b, keep = self._batch(seq, offsets)
        n = len(offsets) - 1
        ln = np.zeros(int(keep[1][-1] - keep[1][0]), dtype=np.uint32)
        mx = np.zeros(n, dtype=np.uint32)
        hits = np.zeros(n, dtype=np.uint32)
        _chk(self._L.moni_pml_batch(self._h, C.byref(b), thr, ln.ctypes.data, mx.ctypes.data, hits.ctypes.data), "moni_pml_batch")
        self.n_reads = n
        return ln, mx, hits

    def pml_run(self, thr: int = 25):
        """moni_pml_run over the batch made resident by upload(): device only, the results wait for pml_fetch()"""
        _chk(self._L.moni_pml_run(self._h, thr), "moni_pml_run")

    def pml_fetch(self, want_lengths: bool = True):
        """(lengths or None, read_max, read_hits) of the last pml_run(); the arrays are sized by what the library says that run covered
        (moni_pml_sizes), whichever calls made its batch resident"""
        nr, total = C.c_uint64(), C.c_uint64()
        _chk(self._L.moni_pml_sizes(self._h, C.byref(nr), C.byref(total)), "moni_pml_sizes")
        ln = np.zeros(total.value, dtype=np.uint32) if want_lengths else None
        mx = np.zeros(nr.value, dtype=np.uint32)
        hits = np.zeros(nr.value, dtype=np.uint32)
        _chk(self._L.moni_pml_fetch(self._h, ln.ctypes.data if want_lengths else None, mx.ctypes.data, hits.ctypes.data), "moni_pml_fetch")
        return ln, mx, hits

    def _screen_params(self, overrides) -> "ScreenParamsC":
        p = ScreenParamsC()
        self._L.moni_screen_params_default(C.byref(p))
        for k, v in overrides.items():
            setattr(p, k, v)
        return p

    def screen_batch(self, seq: np.ndarray, offsets: np.ndarray, **overrides):
        """read screening (moni_screen_batch): one record per read (SCREEN_RES_DTYPE: n_win, n_pos[2], d_max[2], max_pml[2], flags) - the windows
        of pseudo-matching lengths of either strand against those of the read reversed.  overrides: fields of moni_screen_params_t (window,
        min_win, ks_num, ks_den, strands)."""
        b, keep = self._batch(seq, offsets)
        n = len(offsets) - 1
        p = self._screen_params(overrides)
        res = np.zeros(n, dtype=SCREEN_RES_DTYPE)
        _chk(self._L.moni_screen_batch(self._h, C.byref(b), C.byref(p), res.ctypes.data if n else None), "moni_screen_batch")
        self.n_reads = n
        return res

    def screen_run(self, **overrides):
        """moni_screen_run over the batch made resident by upload(): device only, the records wait for screen_fetch()"""
        p = self._screen_params(overrides)
        _chk(self._L.moni_screen_run(self._h, C.byref(p)), "moni_screen_run")

    def screen_fetch(self) -> np.ndarray:
        """the records of the last screen_run(), as many as the library says that run covered (moni_screen_sizes)"""
        nr = C.c_uint64()
        _chk(self._L.moni_screen_sizes(self._h, C.byref(nr)), "moni_screen_sizes")
        res = np.zeros(nr.value, dtype=SCREEN_RES_DTYPE)
        _chk(self._L.moni_screen_fetch(self._h, res.ctypes.data if nr.value else None), "moni_screen_fetch")
        return res

    def bgzf_compress(self, data, block_size: int = 65280, level: int = 1, eof: bool = False, reserved: int = 0):
        """moni_bgzf_compress: `data` (bytes, or a uint8 array) as a concatenation of BGZF blocks of at most block_size bytes of it each, with the
        end-of-file block where asked for.  Returns (bytes, stats: the fields of moni_bgzf_stats_t)."""
        buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
        p = BgzfParamsC()
        self._L.moni_bgzf_params_default(C.byref(p))
        p.block_size, p.level, p.eof, p.reserved = block_size, level, 1 if eof else 0, reserved
        out, n, st = C.c_void_p(), C.c_uint64(), BgzfStatsC()
        _chk(self._L.moni_bgzf_compress(self._h, buf.ctypes.data if buf.size else None, buf.size, C.byref(p), C.byref(out), C.byref(n), C.byref(st)),
             "moni_bgzf_compress")
        return C.string_at(out.value, n.value) if n.value else b"", {k: getattr(st, k) for k, _ in BgzfStatsC._fields_}

    def bgzf_inflate(self, data, check_crc: bool = True, reserved: int = 0, rc_only: bool = False):
        """moni_bgzf_inflate: the text of `data` (bytes, or a uint8 array: whole BGZF members).  Returns (bytes, stats: the fields of
        moni_inflate_stats_t); with rc_only (the return code, out_len, stats), raising nothing."""
        buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
        p = InflateParamsC()
        self._L.moni_inflate_params_default(C.byref(p))
        p.check_crc, p.reserved[0] = 1 if check_crc else 0, reserved
        out, n, st = C.c_void_p(), C.c_uint64(), InflateStatsC()
        rc = self._L.moni_bgzf_inflate(self._h, buf.ctypes.data if buf.size else None, buf.size, C.byref(p), C.byref(out), C.byref(n), C.byref(st))
        stats = {k: getattr(st, k) for k, _ in InflateStatsC._fields_}
        if rc_only:
            return rc, n.value, stats
        _chk(rc, "moni_bgzf_inflate")
        return C.string_at(out.value, n.value) if n.value else b"", stats

    def bam_in_reset(self):
        """moni_bam_in_reset: the next bam_in_feed starts a file"""
        _chk(self._L.moni_bam_in_reset(self._h), "moni_bam_in_reset")

    def bam_in_feed(self, data, paired: bool = False, last: bool = False, check_crc: bool = True, rc_only: bool = False):
        """moni_bam_in_feed: whole BGZF members of a BAM file (bytes, or a uint8 array) behind what the calls before left over.  Returns
        (text1, text2, reads or pairs, stats: the fields of moni_bamin_stats_t with the inflater's under 'inflate' and t_kernel as a dict by
        BAMIN_PHASES); with rc_only the return code comes first and nothing is raised."""
        buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
        p = BamInParamsC()
        self._L.moni_bamin_params_default(C.byref(p))
        p.paired, p.check_crc = 1 if paired else 0, 1 if check_crc else 0
        t1, t2, n1, n2, nr, st = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_uint64(), BamInStatsC()
        rc = self._L.moni_bam_in_feed(self._h, buf.ctypes.data if buf.size else None, buf.size, C.byref(p), 1 if last else 0, C.byref(t1), C.byref(n1), C.byref(t2),
                                      C.byref(n2), C.byref(nr), C.byref(st))
        stats = {k: getattr(st, k) for k, _ in BamInStatsC._fields_ if k not in ("inflate", "t_kernel")}
        stats["inflate"] = {k: getattr(st.inflate, k) for k, _ in InflateStatsC._fields_}
        stats["t_kernel"] = dict(zip(BAMIN_PHASES, st.t_kernel))
        out = (C.string_at(t1.value, n1.value) if n1.value else b"", C.string_at(t2.value, n2.value) if n2.value else b"", nr.value, stats)
        if rc_only:
            return (rc,) + out
        _chk(rc, "moni_bam_in_feed")
        return out

    def bam_set_header(self, text) -> bytes:
        """moni_bam_set_header: the dictionary of the @SQ lines of `text` (bytes or str) for this context's bam_records; returns the uncompressed
        BAM header."""
        t = text.encode() if isinstance(text, str) else bytes(text)
        out, n = C.c_void_p(), C.c_uint64()
        _chk(self._L.moni_bam_set_header(self._h, t, len(t), C.byref(out), C.byref(n)), "moni_bam_set_header")
        return C.string_at(out.value, n.value)

    def bam_records(self, data, block_size: int = 65280, level: int = 1, eof: bool = False, raw: bool = False):
        """moni_bam_records: the SAM lines `data` (bytes, or a uint8 array) as BAM records in BGZF blocks, or with raw the records themselves.
        Returns (bytes, stats: the fields of moni_bam_stats_t); raises BamBadLine, with the stats, where a line is a bad line."""
        buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
        p = BamParamsC()
        self._L.moni_bam_params_default(C.byref(p))
        p.block_size, p.level, p.eof, p.raw = block_size, level, 1 if eof else 0, 1 if raw else 0
        out, n, st = C.c_void_p(), C.c_uint64(), BamStatsC()
        rc = self._L.moni_bam_records(self._h, buf.ctypes.data if buf.size else None, buf.size, C.byref(p), C.byref(out), C.byref(n), C.byref(st))
        stats = {k: getattr(st, k) for k, _ in BamStatsC._fields_ if k != "pad"}
        if rc == -22 and st.bad_lines:
            raise BamBadLine(stats)
        _chk(rc, "moni_bam_records")
        return C.string_at(out.value, n.value) if n.value else b"", stats

    def bam_sorted_run(self, data):
        """moni_bam_sorted_run: the SAM lines `data` as raw BAM records in coordinate order.  Returns (records: bytes, keys[n] ascending,
        offs[n + 1], stats: the fields of moni_bam_sort_stats_t); raises BamBadLine, with the encoder's figures, where a line is a bad line."""
        buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
        rec, rl, keys, offs, n, st = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_void_p(), C.c_uint64(), BamSortStatsC()
        rc = self._L.moni_bam_sorted_run(self._h, buf.ctypes.data if buf.size else None, buf.size, C.byref(rec), C.byref(rl), C.byref(keys), C.byref(offs),
                                         C.byref(n), C.byref(st))
        stats = {k: getattr(st, k) for k, _ in BamSortStatsC._fields_ if k != "pad"}
        if rc == -22 and st.bad_records:
            raise BamBadLine(dict(bad_lines=st.bad_records, first_bad_line=st.first_bad_record, bad_reason=st.bad_reason))
        _chk(rc, "moni_bam_sorted_run")
        k = np.frombuffer(C.string_at(keys.value, 8 * n.value), dtype=np.uint64) if n.value else np.zeros(0, np.uint64)
        o = np.frombuffer(C.string_at(offs.value, 8 * (n.value + 1)), dtype=np.uint64)
        return C.string_at(rec.value, rl.value) if rl.value else b"", k, o, stats

    def bam_sort(self, records, offs, block_size: int = 65280, level: int = 1, eof: bool = False, raw: bool = False):
        """moni_bam_sort: raw BAM records (bytes or a uint8 array; record i at offs[i] .. offs[i + 1]) sorted stably by coordinate and deflated, or
        with raw as they are.  Returns (bytes, ents: BAM_ENT_DTYPE[n] in sorted order, stats); raises BamBadRecord, with the stats, on a bad record."""
        buf = np.frombuffer(records, dtype=np.uint8) if isinstance(records, (bytes, bytearray, memoryview)) else np.ascontiguousarray(records, dtype=np.uint8)
        o = np.ascontiguousarray(offs, dtype=np.uint64)
        n = max(len(o) - 1, 0)
        p = BamParamsC()
        self._L.moni_bam_params_default(C.byref(p))
        p.block_size, p.level, p.eof, p.raw = block_size, level, 1 if eof else 0, 1 if raw else 0
        out, ol, ents, st = C.c_void_p(), C.c_uint64(), C.c_void_p(), BamSortStatsC()
        rc = self._L.moni_bam_sort(self._h, buf.ctypes.data if buf.size else None, buf.size, o.ctypes.data if o.size else None, n, C.byref(p), C.byref(out),
                                   C.byref(ol), C.byref(ents), C.byref(st))
        stats = {k: getattr(st, k) for k, _ in BamSortStatsC._fields_ if k != "pad"}
        if rc == -22 and st.bad_records:
            raise BamBadRecord(stats)
        _chk(rc, "moni_bam_sort")
        e = np.frombuffer(C.string_at(ents.value, BAM_ENT_DTYPE.itemsize * n), dtype=BAM_ENT_DTYPE) if n else np.zeros(0, BAM_ENT_DTYPE)
        return C.string_at(out.value, ol.value) if ol.value else b"", e, stats

    def bam_sorted_run_dup(self, data, paired):
        """moni_bam_sorted_run_dup: bam_sorted_run's four results, then the run's entries (BAM_DUP_DTYPE, input order) and the call's stats
        (those of the run, then entries, pairs, fragments, t_sig, t_entry).  Raises BamBadLine for a bad line, BamBadRecord for a record that
        duplicate marking refuses (SEQ, CLIP, MATE)."""
        buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
        rec, rl, keys, offs, n, st = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_void_p(), C.c_uint64(), BamRunDupStatsC()
        dups, nd = C.c_void_p(), C.c_uint64()
        rc = self._L.moni_bam_sorted_run_dup(self._h, buf.ctypes.data if buf.size else None, buf.size, int(paired), C.byref(rec), C.byref(rl), C.byref(keys),
                                             C.byref(offs), C.byref(n), C.byref(dups), C.byref(nd), C.byref(st))
        stats = {k: getattr(st.run, k) for k, _ in BamSortStatsC._fields_ if k != "pad"}
        stats.update({k: getattr(st, k) for k, _ in BamRunDupStatsC._fields_ if k not in ("run", "pad")})
        if rc == -22 and st.run.bad_records:
            if st.bad_is_record:
                raise BamBadRecord(stats)
            raise BamBadLine(dict(bad_lines=st.run.bad_records, first_bad_line=st.run.first_bad_record, bad_reason=st.run.bad_reason))
        _chk(rc, "moni_bam_sorted_run_dup")
        k = np.frombuffer(C.string_at(keys.value, 8 * n.value), dtype=np.uint64) if n.value else np.zeros(0, np.uint64)
        o = np.frombuffer(C.string_at(offs.value, 8 * (n.value + 1)), dtype=np.uint64)
        d = np.frombuffer(C.string_at(dups.value, BAM_DUP_DTYPE.itemsize * nd.value), dtype=BAM_DUP_DTYPE) if nd.value else np.zeros(0, BAM_DUP_DTYPE)
        return C.string_at(rec.value, rl.value) if rl.value else b"", k, o, d, stats

    def bam_dup_resolve(self, dups, n_records):
        """moni_bam_dup_resolve: dups[r] the entries of run r (BAM_DUP_DTYPE), n_records[r] its records.  Returns ([marks of run r: uint8], stats);
        raises BamBadEntry where an entry points outside its run."""
        R = len(dups)
        ds = [np.ascontiguousarray(d, dtype=BAM_DUP_DTYPE) for d in dups]
        nd = np.array([len(d) for d in ds], dtype=np.uint64)
        nr = np.array([int(x) for x in n_records], dtype=np.uint64)
        marks = [np.full(int(x), 0xEE, dtype=np.uint8) for x in nr]
        dp = (C.c_void_p * max(R, 1))(*[d.ctypes.data if d.size else None for d in ds])
        mp = (C.c_void_p * max(R, 1))(*[m.ctypes.data if m.size else None for m in marks])
        st = BamDupStatsC()
        rc = self._L.moni_bam_dup_resolve(self._h, dp if R else None, nd.ctypes.data if R else None, nr.ctypes.data if R else None, R, mp if R else None, C.byref(st))
        stats = {k: getattr(st, k) for k, _ in BamDupStatsC._fields_}
        if rc == -22 and st.bad_entries:
            raise BamBadEntry(stats)
        _chk(rc, "moni_bam_dup_resolve")
        return marks, stats

    def bam_sort_marked(self, records, offs, marks, block_size: int = 65280, level: int = 1, eof: bool = False, raw: bool = False):
        """moni_bam_sort_marked: bam_sort with marks[n] (uint8, or None) beside the input records: a marked record leaves with flag | 0x400"""
        buf = np.frombuffer(records, dtype=np.uint8) if isinstance(records, (bytes, bytearray, memoryview)) else np.ascontiguousarray(records, dtype=np.uint8)
        o = np.ascontiguousarray(offs, dtype=np.uint64)
        n = max(len(o) - 1, 0)
        m = None if marks is None else np.ascontiguousarray(marks, dtype=np.uint8)
        if m is not None and m.size != n:
            raise ValueError("bam_sort_marked: one mark per record")
        p = BamParamsC()
        self._L.moni_bam_params_default(C.byref(p))
        p.block_size, p.level, p.eof, p.raw = block_size, level, 1 if eof else 0, 1 if raw else 0
        out, ol, ents, st = C.c_void_p(), C.c_uint64(), C.c_void_p(), BamSortStatsC()
        rc = self._L.moni_bam_sort_marked(self._h, buf.ctypes.data if buf.size else None, buf.size, o.ctypes.data if o.size else None, n,
                                          m.ctypes.data if m is not None and m.size else (None if m is None or n else m.ctypes.data), C.byref(p), C.byref(out),
                                          C.byref(ol), C.byref(ents), C.byref(st))
        stats = {k: getattr(st, k) for k, _ in BamSortStatsC._fields_ if k != "pad"}
        if rc == -22 and st.bad_records:
            raise BamBadRecord(stats)
        _chk(rc, "moni_bam_sort_marked")
        e = np.frombuffer(C.string_at(ents.value, BAM_ENT_DTYPE.itemsize * n), dtype=BAM_ENT_DTYPE) if n else np.zeros(0, BAM_ENT_DTYPE)
        return C.string_at(out.value, ol.value) if ol.value else b"", e, stats

    def _locate_params(self, strands: int, max_occ: int) -> "LocateParamsC":
        p = LocateParamsC()
        self._L.moni_locate_params_default(C.byref(p))
        p.strands, p.max_occ = strands, max_occ
        return p

    def locate_batch(self, seq: np.ndarray, offsets: np.ndarray, strands: int = 1, max_occ: int = 0):
        """exact-match count and locate (moni_locate_batch): (res, pos, seq, seq_off) - res[i * strands + s] (LOCATE_RES_DTYPE: count, sa_lo,
        occ_off, n_occ, matched) of pattern i on strand s, and the text position, sequence index and offset inside the sequence of the
        n_occ = min(count, max_occ) occurrences kept of each, at res["occ_off"]"""
        b, keep = self._batch(seq, offsets)
        n = len(offsets) - 1
        p = self._locate_params(strands, max_occ)
        res = np.zeros(n * strands, dtype=LOCATE_RES_DTYPE)
        hp, hs, ho, no = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
        _chk(self._L.moni_locate_batch(self._h, C.byref(b), C.byref(p), res.ctypes.data, C.byref(hp), C.byref(hs), C.byref(ho), C.byref(no)), "moni_locate_batch")
        self.n_reads = n
        try:
            k = no.value
            take = lambda h, dt: np.frombuffer(C.string_at(h, k * np.dtype(dt).itemsize), dtype=dt).copy() if k else np.zeros(0, dtype=dt)
            return res, take(hp, np.uint64), take(hs, np.uint32), take(ho, np.uint64)
        finally:
            for h in (hp, hs, ho):
                self._L.moni_free(h)

    def locate_run(self, strands: int = 1, max_occ: int = 0):
        """moni_locate_run over the batch made resident by upload(): device only, the results wait for locate_fetch()"""
        p = self._locate_params(strands, max_occ)
        _chk(self._L.moni_locate_run(self._h, C.byref(p)), "moni_locate_run")

    def locate_fetch(self, want_occ: bool = True):
        """(res, pos, seq, seq_off) of the last locate_run(), sized by moni_locate_sizes; want_occ=False fetches the records alone (the three
        arrays come back empty)"""
        nt, no = C.c_uint64(), C.c_uint64()
        _chk(self._L.moni_locate_sizes(self._h, C.byref(nt), C.byref(no)), "moni_locate_sizes")
        k = no.value if want_occ else 0
        res = np.zeros(nt.value, dtype=LOCATE_RES_DTYPE)
        pos, sq, so = np.zeros(k, dtype=np.uint64), np.zeros(k, dtype=np.uint32), np.zeros(k, dtype=np.uint64)
        _chk(self._L.moni_locate_fetch(self._h, res.ctypes.data, pos.ctypes.data if k else None, sq.ctypes.data if k else None, so.ctypes.data if k else None),
             "moni_locate_fetch")
        return res, pos, sq, so

    def _seqcount_params(self, strands: int, max_walk: int) -> "SeqcountParamsC":
        p = SeqcountParamsC()
        self._L.moni_seqcount_params_default(C.byref(p))
        p.strands, p.max_walk = strands, max_walk
        return p

    def seqcount_batch(self, seq: np.ndarray, offsets: np.ndarray, strands: int = 1, max_walk: int = 1 << 20):
        """per-sequence occurrence counts (moni_seqcount_batch): (res, counts) - res[i * strands + s] (SEQCOUNT_RES_DTYPE: count, sa_lo, matched,
        n_seqs, walked, n_segs) of pattern i on strand s and counts[i * strands + s, q], its occurrences that start in sequence q; a task with
        count > max_walk (0: no limit) is not walked and its row is zero"""
        b, keep = self._batch(seq, offsets)
        n = len(offsets) - 1
        p = self._seqcount_params(strands, max_walk)
        res = np.zeros(n * strands, dtype=SEQCOUNT_RES_DTYPE)
        _chk(self._L.moni_seqcount_batch(self._h, C.byref(b), C.byref(p), res.ctypes.data, None), "moni_seqcount_batch")
        self.n_reads = n
        if not n:                                    # nothing was run: no row, and no width to ask for
            return res, np.zeros((0, 0), dtype=np.uint64)
        counts = np.zeros(self.seqcount_sizes(), dtype=np.uint64)          # the table's width is the index's: asked once the run has happened
        _chk(self._L.moni_seqcount_fetch(self._h, None, counts.ctypes.data), "moni_seqcount_fetch")
        return res, counts

    def seqcount_run(self, strands: int = 1, max_walk: int = 1 << 20):
        """moni_seqcount_run over the batch made resident by upload(): device only, the results wait for seqcount_fetch()"""
        p = self._seqcount_params(strands, max_walk)
        _chk(self._L.moni_seqcount_run(self._h, C.byref(p)), "moni_seqcount_run")

    def seqcount_sizes(self):
        """(n_tasks, n_seq) of the last seqcount_run()"""
        nt, ns = C.c_uint64(), C.c_uint32()
        _chk(self._L.moni_seqcount_sizes(self._h, C.byref(nt), C.byref(ns)), "moni_seqcount_sizes")
        return nt.value, ns.value

    def seqcount_fetch(self, want_counts: bool = True):
        """(res, counts) of the last seqcount_run(), sized by moni_seqcount_sizes; want_counts=False fetches the records alone (counts is None)"""
        nt, ns = self.seqcount_sizes()
        res = np.zeros(nt, dtype=SEQCOUNT_RES_DTYPE)
        counts = np.zeros((nt, ns), dtype=np.uint64) if want_counts else None
        _chk(self._L.moni_seqcount_fetch(self._h, res.ctypes.data, counts.ctypes.data if want_counts else None), "moni_seqcount_fetch")
        return res, counts

    def _loci_params(self, strands: int, lift: int, max_walk: int, max_total: Optional[int]) -> "LociParamsC":
        p = LociParamsC()
        self._L.moni_loci_params_default(C.byref(p))
        p.strands, p.lift, p.max_walk = strands, lift, max_walk
        if max_total is not None:
            p.max_total = max_total
        return p

    def loci_batch(self, seq: np.ndarray, offsets: np.ndarray, strands: int = 1, lift: int = 1, max_walk: int = 1 << 20, max_total: Optional[int] = None):
        """reference loci (moni_loci_batch): (res, lpos, lseq, lseq_off, support) - res[i * strands + s] (LOCI_RES_DTYPE: count, sa_lo, loci_off, n_loci,
        matched, walked, n_segs) of pattern i on strand s, and at res["loci_off"] its n_loci distinct lifted positions (lift=0: text positions) in
        ascending order, the sequence each lies in, the offset inside it and the number of occurrences that land there"""
        b, keep = self._batch(seq, offsets)
        n = len(offsets) - 1
        p = self._loci_params(strands, lift, max_walk, max_total)
        res = np.zeros(n * strands, dtype=LOCI_RES_DTYPE)
        hp, hs, ho, hu, nl = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
        _chk(self._L.moni_loci_batch(self._h, C.byref(b), C.byref(p), res.ctypes.data, C.byref(hp), C.byref(hs), C.byref(ho), C.byref(hu), C.byref(nl)), "moni_loci_batch")
        self.n_reads = n
        try:
            k = nl.value
            take = lambda h, dt: np.frombuffer(C.string_at(h, k * np.dtype(dt).itemsize), dtype=dt).copy() if k else np.zeros(0, dtype=dt)
            return res, take(hp, np.uint64), take(hs, np.uint32), take(ho, np.uint64), take(hu, np.uint64)
        finally:
            for h in (hp, hs, ho, hu):
                self._L.moni_free(h)

    def loci_run(self, strands: int = 1, lift: int = 1, max_walk: int = 1 << 20, max_total: Optional[int] = None):
        """moni_loci_run over the batch made resident by upload(): device only, the results wait for loci_fetch()"""
        p = self._loci_params(strands, lift, max_walk, max_total)
        _chk(self._L.moni_loci_run(self._h, C.byref(p)), "moni_loci_run")

    def loci_sizes(self):
        """(n_tasks, n_loci) of the last loci_run()"""
        nt, nl = C.c_uint64(), C.c_uint64()
        _chk(self._L.moni_loci_sizes(self._h, C.byref(nt), C.byref(nl)), "moni_loci_sizes")
        return nt.value, nl.value

    def loci_fetch(self, want_loci: bool = True):
        """(res, lpos, lseq, lseq_off, support) of the last loci_run(), sized by moni_loci_sizes; want_loci=False fetches the records alone (the four
        arrays come back empty)"""
        nt, nl = self.loci_sizes()
        k = nl if want_loci else 0
        res = np.zeros(nt, dtype=LOCI_RES_DTYPE)
        lp, ls, lo, su = np.zeros(k, dtype=np.uint64), np.zeros(k, dtype=np.uint32), np.zeros(k, dtype=np.uint64), np.zeros(k, dtype=np.uint64)
        ptr = lambda a: a.ctypes.data if k else None
        _chk(self._L.moni_loci_fetch(self._h, res.ctypes.data, ptr(lp), ptr(ls), ptr(lo), ptr(su)), "moni_loci_fetch")
        return res, lp, ls, lo, su

    def _approx_params(self, strands, k, max_hits, max_occ, chunk_len, max_steps) -> "ApproxParamsC":
        p = ApproxParamsC()
        self._L.moni_approx_params_default(C.byref(p))
        p.strands, p.k, p.max_hits, p.max_occ = strands, k, max_hits, max_occ
        if chunk_len is not None:
            p.chunk_len = chunk_len
        if max_steps is not None:
            p.max_steps = max_steps
        return p

    def approx_batch(self, seq: np.ndarray, offsets: np.ndarray, strands: int = 1, k: int = 1, max_hits: int = 0, max_occ: int = 0, chunk_len: Optional[int] = None,
                     max_steps: Optional[int] = None):
        """k-mismatch count and locate (moni_approx_batch): (res, hits, pos, seq, seq_off) - res[i * strands + s] (APPROX_RES_DTYPE: cnt[4], the text
        positions at distance 0..3; n_hits, hit_off, n_kept, complete, matched) of pattern i on strand s; hits (APPROX_HIT_DTYPE: task, n_mis, n_occ,
        sa_lo, count, occ_off) the n_kept = min(n_hits, max_hits) matching strings kept of each task at res["hit_off"], sorted by (n_mis, sa_lo); and
        the text position, sequence index and offset inside the sequence of the n_occ = min(count, max_occ) positions kept of each hit, at
        hits["occ_off"].  chunk_len: pattern places per piece of a search tree, max_steps: backward-search steps per piece (None: the library's defaults; max_steps 0: no limit)."""
        b, keep = self._batch(seq, offsets)
        n = len(offsets) - 1
        p = self._approx_params(strands, k, max_hits, max_occ, chunk_len, max_steps)
        res = np.zeros(n * strands, dtype=APPROX_RES_DTYPE)
        hh, hp, hs, ho, nh, no = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        _chk(self._L.moni_approx_batch(self._h, C.byref(b), C.byref(p), res.ctypes.data, C.byref(hh), C.byref(hp), C.byref(hs), C.byref(ho), C.byref(nh), C.byref(no)),
             "moni_approx_batch")
        self.n_reads = n
        try:
            take = lambda h, k_, dt: np.frombuffer(C.string_at(h, k_ * np.dtype(dt).itemsize), dtype=dt).copy() if k_ else np.zeros(0, dtype=dt)
            return res, take(hh, nh.value, APPROX_HIT_DTYPE), take(hp, no.value, np.uint64), take(hs, no.value, np.uint32), take(ho, no.value, np.uint64)
        finally:
            for h in (hh, hp, hs, ho):
                self._L.moni_free(h)

    def approx_run(self, strands: int = 1, k: int = 1, max_hits: int = 0, max_occ: int = 0, chunk_len: Optional[int] = None, max_steps: Optional[int] = None):
        """moni_approx_run over the batch made resident by upload(): device only, the results wait for approx_fetch()"""
        p = self._approx_params(strands, k, max_hits, max_occ, chunk_len, max_steps)
        _chk(self._L.moni_approx_run(self._h, C.byref(p)), "moni_approx_run")

    def approx_sizes(self):
        """(n_tasks, hits kept, positions) of the last approx_run()"""
        nt, nh, no = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _chk(self._L.moni_approx_sizes(self._h, C.byref(nt), C.byref(nh), C.byref(no)), "moni_approx_sizes")
        return nt.value, nh.value, no.value

    def approx_fetch(self, want_hits: bool = True):
        """(res, hits, pos, seq, seq_off) of the last approx_run(), sized by moni_approx_sizes; want_hits=False fetches the records alone (the four
        arrays come back empty)"""
        nt, nh, no = self.approx_sizes()
        if not want_hits:
            nh = no = 0
        res = np.zeros(nt, dtype=APPROX_RES_DTYPE)
        hits = np.zeros(nh, dtype=APPROX_HIT_DTYPE)
        pos, sq, so = np.zeros(no, dtype=np.uint64), np.zeros(no, dtype=np.uint32), np.zeros(no, dtype=np.uint64)
        _chk(self._L.moni_approx_fetch(self._h, res.ctypes.data, hits.ctypes.data if nh else None, pos.ctypes.data if no else None, sq.ctypes.data if no else None,
                                       so.ctypes.data if no else None), "moni_approx_fetch")
        return res, hits, pos, sq, so

    def ms_lengths_batch(self, seq: np.ndarray, offsets: np.ndarray):
        """legacy `moni ms`: (pointers, lengths) of the forward strand of every read"""
        b, keep = self._batch(seq, offsets)
        total = int(keep[1][-1] - keep[1][0])
        ptr = np.empty(total, dtype=np.uint64)
        ln = np.empty(total, dtype=np.uint64)
        _chk(self._L.moni_ms_lengths_batch(self._h, C.byref(b), ptr.ctypes.data, ln.ctypes.data), "moni_ms_lengths_batch")
        self.n_reads = len(offsets) - 1
        return ptr, ln

    def ms_long_batch(self, seq: np.ndarray, offsets: np.ndarray, seg_len: int = None, overlap: int = None, want_pointers: bool = True, want_lengths: bool = True):
        """matching statistics of genome-length patterns (moni_ms_long_batch): (pointers or None, lengths or None, stats) in the layout of
        ms_lengths_batch.  The lengths are identical to ms_lengths_batch's; the pointers are valid but may differ where a pattern was cut into
        segments (seg_len >= the longest pattern: identical).  The call replaces the resident batch: upload() again before any *_run call."""
        b, keep = self._batch(seq, offsets)
        total = int(keep[1][-1] - keep[1][0])
        p = MslongParamsC()
        self._L.moni_mslong_params_default(C.byref(p))
        if seg_len is not None:
            p.seg_len = seg_len
        if overlap is not None:
            p.overlap = overlap
        ptr = np.empty(total, dtype=np.uint64) if want_pointers else None
        ln = np.empty(total, dtype=np.uint64) if want_lengths else None
        st = MslongStatsC()
        _chk(self._L.moni_ms_long_batch(self._h, C.byref(b), C.byref(p), ptr.ctypes.data if want_pointers else None, ln.ctypes.data if want_lengths else None, C.byref(st)),
             "moni_ms_long_batch")
        self.n_reads = 0
        return ptr, ln, {f: getattr(st, f) for f, _ in MslongStatsC._fields_}

    def report_mems_batch(self, seq, offsets, names, name_off, quals=None, **overrides) -> bytes:
        b, keep = self._batch(seq, offsets)
        names = np.ascontiguousarray(names, dtype=np.uint8)
        name_off = np.ascontiguousarray(name_off, dtype=np.uint64)
        if quals is not None:
            quals = np.ascontiguousarray(quals, dtype=np.uint8)
        prm = AlignParamsC()
        self._L.moni_align_params_default(C.byref(prm))
        for k, v in overrides.items():
            setattr(prm, k, v)
        out, ln = C.c_void_p(), C.c_uint64()
        _chk(self._L.moni_report_mems_batch(self._h, C.byref(b), names.ctypes.data, name_off.ctypes.data, quals.ctypes.data if quals is not None else None,
                                            C.byref(prm), C.byref(out), C.byref(ln)), "moni_report_mems_batch")
        self.n_reads = len(offsets) - 1
        try:
            return C.string_at(out, ln.value)
        finally:
            self._L.moni_free(out)

    def sam_header(self) -> bytes:
        out = C.c_void_p()
        ln = C.c_uint64()
        _chk(self._L.moni_sam_header(self.index._h, C.byref(out), C.byref(ln)), "moni_sam_header")
        try:
            return C.string_at(out, ln.value)
        finally:
            self._L.moni_free(out)

    def kernel_ms(self, which: int) -> float:
        v = C.c_float()
        _chk(self._L.moni_last_kernel_ms(self._h, which, C.byref(v)), "moni_last_kernel_ms")
        return float(v.value)

    def counters(self) -> np.ndarray:
        out = np.zeros(4, dtype=np.uint64)
        _chk(self._L.moni_last_counters(self._h, out.ctypes.data), "moni_last_counters")
        return out

    def seed_occ_stats(self) -> Dict[str, int]:
        """the occurrence stage of the last seed_run (moni_seed_occ_stats)"""
        out = np.zeros(6, dtype=np.uint64)
        _chk(self._L.moni_seed_occ_stats(self._h, out.ctypes.data), "moni_seed_occ_stats")
        return dict(zip(("long_seeds", "overflow_used", "overflow_cap", "count_passes", "long_launches", "compactions"), (int(v) for v in out)))

    def seed_prefilter(self, mode: int) -> None:
        """the strand prefilter of the seeding stage: 0 off, 1 in the align and paired paths (default), 2 in seed_run too (moni_seed_prefilter)"""
        _chk(self._L.moni_seed_prefilter(self._h, int(mode)), "moni_seed_prefilter")

    def seed_prefilter_stats(self) -> Dict[str, float]:
        """the filter in the last seeding run (moni_seed_prefilter_stats)"""
        out = np.zeros(4, dtype=np.uint64)
        _chk(self._L.moni_seed_prefilter_stats(self._h, out.ctypes.data), "moni_seed_prefilter_stats")
        return {"tasks": int(out[0]), "skipped": int(out[1]), "lookups": int(out[2]), "density": float(out[3]) / 1e6}


    def ms_leap_stats(self) -> Dict[str, int]:
        """the leaps of the walk in the last seeding run (moni_ms_leap_stats); stride 0: the index has no table"""
        out = np.zeros(4, dtype=np.uint64)
        _chk(self._L.moni_ms_leap_stats(self._h, out.ctypes.data), "moni_ms_leap_stats")
        return dict(zip(("leaps", "steps_leapt", "comparisons", "stride"), (int(v) for v in out)))


def ldx_info(path: str):
    n_seq, u, w, has_w = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
    _chk(lib().moni_ldx_info(path.encode(), C.byref(n_seq), C.byref(u), C.byref(w), C.byref(has_w)), "moni_ldx_info")
    return {"n_seq": n_seq.value, "u": u.value, "w": w.value, "has_w": bool(has_w.value)}


def ldx_rewrite(src: str, dst: str, with_w: bool):
    _chk(lib().moni_ldx_rewrite(src.encode(), dst.encode(), int(with_w)), "moni_ldx_rewrite")


def ldx_write(fi, path: str, with_w: bool = True):
    st = flat_struct(fi)
    _chk(lib().moni_ldx_write(C.byref(st), path.encode(), int(with_w)), "moni_ldx_write")


def ms_file_info(path: str):
    n, r = C.c_uint64(), C.c_uint64()
    _chk(lib().moni_ms_file_info(path.encode(), C.byref(n), C.byref(r)), "moni_ms_file_info")
    return n.value, r.value


def ms_file_read(path: str):
    """<prefix>.thrbv.full.lcp.ms -> dict of the flat arrays (n, r, F, heads, starts, ssa, esa, thr, slcp)."""
    n, r = ms_file_info(path)
    a = {"F": np.zeros(256, np.uint64), "heads": np.zeros(r, np.uint8), "starts": np.zeros(r + 1, np.uint64), "ssa": np.zeros(r, np.uint64),
         "esa": np.zeros(r, np.uint64), "thr": np.zeros(r, np.uint64), "slcp": np.zeros(r, np.uint64)}
    err = C.create_string_buffer(256)
    rc = lib().moni_ms_file_read(path.encode(), r, *[a[k].ctypes.data for k in ("F", "heads", "starts", "ssa", "esa", "thr", "slcp")], err, 256)
    if rc != 0:
        raise RuntimeError("moni_ms_file_read failed with code %d: %s" % (rc, err.value.decode()))
    a["n"], a["r"] = n, r
    return a


def ms_file_write(fi, path: str, without_lcp: bool = False):
    """moni_lcp::serialize (<prefix>.thrbv.full.lcp.ms) or, without_lcp, ms_pointers::serialize (<prefix>.thrbv.full.ms)"""
    st = flat_struct(fi, without_lcp=without_lcp)
    _chk(lib().moni_ms_file_write(C.byref(st), path.encode()), "moni_ms_file_write")


def ldx_lift_batch(path: str, pos: np.ndarray, device: int = 0) -> np.ndarray:
    pos = np.ascontiguousarray(pos, dtype=np.uint64)
    out = np.empty(len(pos), dtype=np.uint64)
    _chk(lib().moni_ldx_lift_batch(path.encode(), device, pos.ctypes.data, len(pos), out.ctypes.data), "moni_ldx_lift_batch")
    return out
