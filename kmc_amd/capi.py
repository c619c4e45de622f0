"""ctypes binding of the C-ABI in include/kmc_hip.h (libkmc_hip.so).

This is the only way Python code (tests, bench.py) reaches the product: through the same `extern "C"` entry points
the C++ worker (kmc_amd/host/kb_sorter_plugin.h) binds. There is no CPU fallback: a missing library or a missing
GPU raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import build as _build

u8p = C.POINTER(C.c_uint8)
u64p = C.POINTER(C.c_uint64)


class KmcHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"kmc_hip error {code}: {msg}")
        self.code = code


class HostBin(C.Structure):
    """struct kmc_hip_host_bin: one bin of a kmc_hip_process_bins_submit call (host pointers)"""

    _fields_ = [
        ("superkmers", C.c_void_p),
        ("size", C.c_uint64),
        ("n_rec", C.c_uint64),
        ("pack_bytes", C.c_void_p),
        ("n_packs", C.c_uint64),
        ("out_suffix", C.c_void_p),
        ("out_capacity", C.c_uint64),
        ("lut", C.c_void_p),
    ]


class BinParams(C.Structure):
    """struct kmc_hip_bin_params (mirrors the CKMCParams fields of kb_sorter.h:165-200)."""

    _fields_ = [
        ("kmer_len", C.c_uint32),
        ("both_strands", C.c_uint32),
        ("cutoff_min", C.c_uint32),
        ("without_output", C.c_uint32),
        ("cutoff_max", C.c_uint64),
        ("counter_max", C.c_uint64),
        ("lut_prefix_len", C.c_uint32),
        ("output_type", C.c_uint32),
    ]


class BinDesc(C.Structure):
    """struct kmc_hip_bin_desc: one device-resident bin of kmc_hip_process_bins_device."""

    _fields_ = [
        ("d_superkmers", C.c_void_p),
        ("size", C.c_uint64),
        ("n_rec", C.c_uint64),
        ("d_pack_start", C.c_void_p),
        ("n_packs", C.c_uint64),
        ("d_out", C.c_void_p),
        ("out_capacity", C.c_uint64),
        ("d_out_bytes", C.c_void_p),
        ("d_lut", C.c_void_p),
        ("d_stats", C.c_void_p),
    ]


class SplitParams(C.Structure):
    """struct kmc_hip_split_params (one part of input text through stage 1, kmc_hip_split_part)."""

    _fields_ = [("kmer_len", C.c_uint32), ("signature_len", C.c_uint32), ("n_bins", C.c_uint32), ("max_x", C.c_uint32), ("both_strands", C.c_uint32),
                ("file_type", C.c_uint32), ("line_cap", C.c_uint64), ("part_kind", C.c_uint32), ("flags", C.c_uint32)]


SPLIT_FILE_BAM = 4  # kmc_hip_split_params.file_type: a part of BAM alignment records (-fbam); ask kmc_hip_split_covers(4) first (3 stays an unknown file type)
SPLIT_HOMOPOLYMER = 1  # KMC_HIP_SPLIT_HOMOPOLYMER: flags bit 0, -hc
SPLIT_ESTIMATE = 4  # KMC_HIP_SPLIT_ESTIMATE: flags bit 2, --opt-out-size (the part's k-mers go to the estimator of kmc_hip_estimate_open)
SPLIT_COVERS_ESTIMATE = 0x102  # KMC_HIP_SPLIT_COVERS_ESTIMATE
SPLIT_COVERS_SMALLK = 0x103  # KMC_HIP_SPLIT_COVERS_SMALLK: kmc_hip_smallk_open / _part / _read / _close (k <= 13 counted on the device)
SMALLK_MAX_K = 13
SPLIT_COVERS_COUNT = 0x105  # KMC_HIP_SPLIT_COVERS_COUNT: kmc_hip_count_open / _part / _finish / _order / _info / _timings / _close (a counting session; 0x104 stays unknown)
SPLIT_COVERS_SIGSTATS = 0x107  # KMC_HIP_SPLIT_COVERS_SIGSTATS: kmc_hip_sigstats_open / _part / _read / _close (stage 0: signature statistics; 0x106 stays unknown)
UNCOVERED = 1  # KMC_HIP_UNCOVERED: malformed text the kernels do not reproduce; nothing was produced
SPLIT_LINE_CAP = (65536 + 1) * 8  # the reference's mem_part_pmm_reads (kmc.h:419, splitter.cpp:18): kmc_hip_split_params.line_cap of a front end
SPLIT_COVERS_HOMOPOLYMER = 0x100  # KMC_HIP_SPLIT_COVERS_HOMOPOLYMER: ask kmc_hip_split_covers before setting the flag (an older library ignores it)


class DbView(C.Structure):
    """struct kmc_hip_db_view: one input of kmc_hip_db_set_op_device, a KMC1 database body on the device"""

    _fields_ = [("d_recs", C.c_void_p), ("n_recs", C.c_uint64), ("d_lut", C.c_void_p), ("lut_prefix_len", C.c_uint32), ("counter_size", C.c_uint32),
                ("cutoff_min", C.c_uint32), ("cutoff_max", C.c_uint64)]


class DbOp(C.Structure):
    """struct kmc_hip_db_op: operation, counter mode and the output's cutoffs of kmc_hip_db_set_op_device"""

    _fields_ = [("op", C.c_uint32), ("counter_op", C.c_uint32), ("cutoff_min", C.c_uint32), ("counter_max", C.c_uint32), ("cutoff_max", C.c_uint64),
                ("out_lut_prefix_len", C.c_uint32)]


# KMC_HIP_DB_*: the operations of `kmc_tools simple` and its -oc counter modes, by the names the command line uses
DB_OPS = {"intersect": 0, "union": 1, "kmers_subtract": 2, "counters_subtract": 3, "reverse_kmers_subtract": 4, "reverse_counters_subtract": 5}
DB_COUNTER_OPS = {"min": 0, "max": 1, "sum": 2, "diff": 3, "left": 4, "right": 5}
class DbExprStep(C.Structure):
    """struct kmc_hip_db_expr_step: one step of the postfix program of kmc_hip_db_expr_device"""

    _fields_ = [("kind", C.c_uint32), ("arg", C.c_uint32)]


DB_EXPR_INPUT = 16  # KMC_HIP_DB_EXPR_INPUT
DB_EXPR_MAX_LEAVES = 16  # KMC_HIP_DB_EXPR_MAX_LEAVES
DB_STATS = ("n_pairs", "n_only_a", "n_only_b", "n_below_min", "n_above_max", "n_written")  # stats[] of kmc_hip_db_set_op_device, in order
DBQ_STATS = ("n_valid_windows", "n_found", "n_cut", "n_invalid_windows")  # stats[] of kmc_hip_db_query_reads_device, in order
DBT_STATS = ("n_cut_in", "n_below_min", "n_above_max", "n_written")  # stats[] of kmc_hip_db_reduce_device and kmc_hip_db_dump_device, in order
DBH_STATS = ("n_cut_in", "n_outside", "n_counted")  # stats[] of kmc_hip_db_histogram_device, in order
DBC_RESULT = ("kind", "ordinal", "n_a", "n_b", "counter_a", "counter_b", "record_a", "record_b")  # result[] of kmc_hip_db_compare_device, in order
DBC_KINDS = ("equal", "counter", "kmer", "a_ended", "b_ended")  # KMC_HIP_DBC_*: result[0]
DBX_STATS = ("n_keys", "n_result", "n_below_min", "n_above_max", "n_written")  # stats[] of kmc_hip_db_expr_device, in order


def make_params(k, both_strands=1, cutoff_min=2, cutoff_max=10**9, counter_max=255, lut_prefix_len=3, output_type=0,
                without_output=0) -> BinParams:
    return BinParams(k, both_strands, cutoff_min, without_output, cutoff_max, counter_max, lut_prefix_len, output_type)


# every symbol include/kmc_hip.h declares (tests check the library exports them all)
SYMBOLS = [
    "kmc_hip_init", "kmc_hip_destroy", "kmc_hip_last_error", "kmc_hip_abi_version", "kmc_hip_backend_kind", "kmc_hip_num_devices", "kmc_hip_num_slots",
    "kmc_hip_device_count",
    "kmc_hip_words", "kmc_hip_counter_size", "kmc_hip_out_rec_bytes", "kmc_hip_lut_entries",
    "kmc_hip_sort_records", "kmc_hip_sort_records_into", "kmc_hip_sort_records_device",
    "kmc_hip_process_bin", "kmc_hip_process_bin_multi", "kmc_hip_process_bins_submit", "kmc_hip_process_bins_wait", "kmc_hip_process_bin_submit", "kmc_hip_process_bin_wait", "kmc_hip_process_bin_device",
    "kmc_hip_process_bins_device", "kmc_hip_order_database_device",
    "kmc_hip_allreduce_stats", "kmc_hip_last_timings", "kmc_hip_scatter_totals", "kmc_hip_local_sort_totals", "kmc_hip_set_hybrid", "kmc_hip_path_counters", "kmc_hip_host_boundary_times", "kmc_hip_reserve_slot",
    "kmc_hip_malloc", "kmc_hip_free", "kmc_hip_memcpy_h2d", "kmc_hip_memcpy_d2h",
    "kmc_hip_host_register", "kmc_hip_host_unregister", "kmc_hip_host_alloc", "kmc_hip_host_free", "kmc_hip_synchronize",
    "kmc_hip_debug_expand", "kmc_hip_debug_compact", "kmc_hip_debug_split_reads",
    "kmc_hip_split_reads_plan", "kmc_hip_split_reads_emit", "kmc_hip_split_reads_free",
    "kmc_hip_split_set_map", "kmc_hip_split_part", "kmc_hip_split_covers", "kmc_hip_estimate_open", "kmc_hip_estimate_read", "kmc_hip_estimate_close",
    "kmc_hip_smallk_open", "kmc_hip_smallk_part", "kmc_hip_smallk_read", "kmc_hip_smallk_close", "kmc_hip_smallk_tally", "kmc_hip_smallk_view_device",
    "kmc_hip_sigstats_open", "kmc_hip_sigstats_part", "kmc_hip_sigstats_read", "kmc_hip_sigstats_close", "kmc_hip_sigstats_allowed",
    "kmc_hip_db_set_op_device", "kmc_hip_db_query_reads_device",
    "kmc_hip_db_reduce_device", "kmc_hip_db_histogram_device", "kmc_hip_db_dump_device",
    "kmc_hip_db_expr_device", "kmc_hip_kff_import_device", "kmc_hip_db_compare_device", "kmc_hip_db_kff_export_device",
    "kmc_hip_count_open", "kmc_hip_count_part", "kmc_hip_count_finish", "kmc_hip_count_order", "kmc_hip_count_info", "kmc_hip_count_timings", "kmc_hip_count_close", "kmc_hip_debug_gather_segments",
    "kmc_hip_bgzf_scan", "kmc_hip_bgzf_inflate_device", "kmc_hip_bgzf_inflate", "kmc_hip_bgzf_last_ms", "kmc_hip_bam_whole_records",
]

_LIB = None


def lib_path() -> str:
    """In-tree libkmc_hip.so; $KMC_HIP_LIB overrides (tuning variants built by tools/build_variants.py)."""
    return os.environ.get("KMC_HIP_LIB") or _build.LIB_HIP


def backend_kind() -> int:
    """0 = the GPU library, 1 = the CPU emulation of the host library (tests), 2 = the mock (tests)"""
    return int(load().kmc_hip_backend_kind())


def require_gpu_backend():
    """bench.py / smoke(): refuse a test build of the library (CPU emulation or mock, see kmc_hip_backend_kind) — numbers and certificates are
    for the GPU library only."""
    kind = load().kmc_hip_backend_kind()
    if kind != 0:
        raise RuntimeError(f"{lib_path()} is a test build of libkmc_hip (backend kind {kind}: CPU emulation / mock), not the GPU library")


def load():
    """dlopen libkmc_hip.so (in-tree). Raises FileNotFoundError when it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    p = lib_path()
    if not os.path.exists(p):
        raise FileNotFoundError(f"{p} is missing — run `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc)")
    L = C.CDLL(p, mode=C.RTLD_GLOBAL)
    vp = C.c_void_p
    L.kmc_hip_init.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
    L.kmc_hip_destroy.argtypes = [vp]
    L.kmc_hip_destroy.restype = None
    L.kmc_hip_last_error.argtypes = [vp]
    L.kmc_hip_last_error.restype = C.c_char_p
    L.kmc_hip_num_devices.argtypes = [vp]
    L.kmc_hip_words.argtypes = [C.c_uint32]
    L.kmc_hip_words.restype = C.c_uint32
    L.kmc_hip_counter_size.argtypes = [C.c_uint64, C.c_uint64]
    L.kmc_hip_counter_size.restype = C.c_uint32
    L.kmc_hip_out_rec_bytes.argtypes = [C.POINTER(BinParams)]
    L.kmc_hip_out_rec_bytes.restype = C.c_uint32
    L.kmc_hip_lut_entries.argtypes = [C.POINTER(BinParams)]
    L.kmc_hip_lut_entries.restype = C.c_uint64
    L.kmc_hip_sort_records.argtypes = [vp, C.c_int, vp, C.c_uint64, C.c_uint32, C.c_uint32]
    L.kmc_hip_sort_records_into.argtypes = [vp, C.c_int, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32]
    L.kmc_hip_sort_records_device.argtypes = [vp, C.c_int, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.kmc_hip_process_bin.argtypes = [vp, C.c_int, C.POINTER(BinParams), vp, C.c_uint64, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64,
                                      u64p, vp, u64p]
    L.kmc_hip_process_bin_multi.argtypes = [vp, C.POINTER(BinParams), vp, C.c_uint64, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, u64p, vp, u64p]
    L.kmc_hip_process_bins_submit.argtypes = [vp, C.c_int, C.c_int, C.POINTER(BinParams), C.POINTER(HostBin), C.c_uint32]
    L.kmc_hip_process_bins_wait.argtypes = [vp, C.c_int, C.c_int, u64p, u64p]
    L.kmc_hip_process_bin_submit.argtypes = [vp, C.c_int, C.c_int, C.POINTER(BinParams), vp, C.c_uint64, C.c_uint64, vp, C.c_uint64,
                                             vp, C.c_uint64, vp]
    L.kmc_hip_process_bin_wait.argtypes = [vp, C.c_int, C.c_int, u64p, u64p]
    L.kmc_hip_process_bin_device.argtypes = [vp, C.c_int, C.POINTER(BinParams), vp, C.c_uint64, C.c_uint64, vp, C.c_uint64, vp,
                                             C.c_uint64, vp, vp, vp, C.c_int]
    L.kmc_hip_allreduce_stats.argtypes = [vp, u64p]
    L.kmc_hip_last_timings.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
    L.kmc_hip_scatter_totals.argtypes = [vp, C.c_int, C.c_int, u64p, C.POINTER(C.c_double), u64p]
    L.kmc_hip_local_sort_totals.argtypes = [vp, C.c_int, C.c_int, u64p, C.POINTER(C.c_double), u64p, u64p, u64p]
    L.kmc_hip_process_bins_device.argtypes = [vp, C.c_int, C.POINTER(BinParams), C.POINTER(BinDesc), C.c_uint64, C.c_int]
    L.kmc_hip_order_database_device.argtypes = [vp, C.c_int, C.POINTER(BinParams), C.POINTER(BinDesc), C.c_uint64, C.c_uint32, vp, C.c_uint64, vp, u64p]
    L.kmc_hip_host_alloc.argtypes = [vp, C.c_uint64, C.POINTER(vp)]
    L.kmc_hip_host_free.argtypes = [vp, vp]
    L.kmc_hip_malloc.argtypes = [vp, C.c_int, C.c_uint64, C.POINTER(vp)]
    L.kmc_hip_free.argtypes = [vp, C.c_int, vp]
    L.kmc_hip_memcpy_h2d.argtypes = [vp, C.c_int, vp, vp, C.c_uint64]
    L.kmc_hip_memcpy_d2h.argtypes = [vp, C.c_int, vp, vp, C.c_uint64]
    L.kmc_hip_host_register.argtypes = [vp, vp, C.c_uint64]
    L.kmc_hip_host_unregister.argtypes = [vp, vp]
    L.kmc_hip_synchronize.argtypes = [vp, C.c_int]
    L.kmc_hip_debug_expand.argtypes = [vp, C.c_int, C.POINTER(BinParams), vp, C.c_uint64, C.c_uint64, vp, C.c_uint64, vp]
    L.kmc_hip_debug_compact.argtypes = [vp, C.c_int, C.POINTER(BinParams), vp, C.c_uint64, vp, C.c_uint64, u64p, vp, u64p]
    L.kmc_hip_debug_split_reads.argtypes = [vp, C.c_int, vp, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.c_uint64, u64p]
    if hasattr(L, "kmc_hip_split_covers"):  # added within ABI version 4: a library without it takes file_type 0 and 1 only, and no flags
        L.kmc_hip_split_covers.argtypes = [C.c_uint32]
    if hasattr(L, "kmc_hip_estimate_open"):  # added within ABI version 4, with KMC_HIP_SPLIT_ESTIMATE
        L.kmc_hip_estimate_open.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32]
        L.kmc_hip_estimate_read.argtypes = [vp, C.c_int, C.c_uint64, C.c_uint64, vp]
        L.kmc_hip_estimate_close.argtypes = [vp, C.c_int]
    if hasattr(L, "kmc_hip_smallk_open"):  # added within ABI version 4: ask kmc_hip_split_covers(SPLIT_COVERS_SMALLK)
        L.kmc_hip_smallk_open.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32]
        L.kmc_hip_smallk_part.argtypes = [vp, C.c_int, C.c_int, C.POINTER(SplitParams), vp, C.c_uint64, u64p, u64p]
        L.kmc_hip_smallk_read.argtypes = [vp, C.c_int, C.c_uint64, C.c_uint64, vp]
        L.kmc_hip_smallk_close.argtypes = [vp, C.c_int]
    bind_sigstats(L)
    bind_smallk_db(L)
    if hasattr(L, "kmc_hip_db_set_op_device"):  # added within ABI version 4
        L.kmc_hip_db_set_op_device.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(DbView), C.POINTER(DbView), C.POINTER(DbOp), vp, C.c_uint64, vp, u64p, u64p]
    if hasattr(L, "kmc_hip_db_query_reads_device"):  # added within ABI version 4
        L.kmc_hip_db_query_reads_device.argtypes = [vp, C.c_int, C.POINTER(DbView), C.c_uint32, C.c_uint32, vp, C.c_uint64, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp, u64p]
    if hasattr(L, "kmc_hip_db_reduce_device"):  # added within ABI version 4, all three together
        L.kmc_hip_db_reduce_device.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(DbView), C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint64, vp, u64p, u64p]
        L.kmc_hip_db_histogram_device.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(DbView), C.c_uint32, C.c_uint32, C.c_uint64, vp, u64p]
        L.kmc_hip_db_dump_device.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(DbView), C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, vp, C.c_uint64, u64p, u64p]
    if hasattr(L, "kmc_hip_db_expr_device"):  # added within ABI version 4
        L.kmc_hip_db_expr_device.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(DbView), C.c_uint32, C.POINTER(DbExprStep), C.c_uint32, C.POINTER(DbOp), vp, C.c_uint64, vp, u64p, u64p]
    if hasattr(L, "kmc_hip_db_compare_device"):  # added within ABI version 4
        L.kmc_hip_db_compare_device.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(DbView), C.POINTER(DbView), u64p]
    if hasattr(L, "kmc_hip_kff_import_device"):  # added within ABI version 4
        L.kmc_hip_kff_import_device.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32, vp, u64p, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint64, vp, u64p]
    if hasattr(L, "kmc_hip_db_kff_export_device"):  # added within ABI version 4
        L.kmc_hip_db_kff_export_device.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(DbView), C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, vp, C.c_uint64]
    bind_count(L)
    bind_bgzf(L)
    _LIB = L
    return L


def bind_count(L):
    """the prototypes of the counting session and its test hook on a loaded library (added within ABI version 4: ask kmc_hip_split_covers(SPLIT_COVERS_COUNT))"""
    if not hasattr(L, "kmc_hip_count_open"):
        return
    vp = C.c_void_p
    L.kmc_hip_split_set_map.argtypes = [vp, C.c_int, vp, C.c_uint32]
    L.kmc_hip_count_open.argtypes = [vp, C.c_int, C.POINTER(SplitParams), C.POINTER(vp)]
    L.kmc_hip_count_part.argtypes = [vp, vp, C.c_int, C.POINTER(SplitParams), vp, C.c_uint64, u64p]
    L.kmc_hip_count_finish.argtypes = [vp, vp, C.POINTER(BinParams), u64p, u64p, u64p]
    L.kmc_hip_count_order.argtypes = [vp, vp, C.c_uint32, C.POINTER(DbView)]
    L.kmc_hip_count_info.argtypes = [vp, vp, u64p]
    L.kmc_hip_count_timings.argtypes = [vp, vp, C.POINTER(C.c_double)]
    L.kmc_hip_count_close.argtypes = [vp, vp]
    L.kmc_hip_count_close.restype = None
    L.kmc_hip_debug_gather_segments.argtypes = [vp, C.c_int, vp, vp, vp, C.c_uint64]


def bind_smallk_db(L):
    """the prototypes of the small-k table's road to a database on a loaded library (added within ABI version 4: ask kmc_hip_split_covers(SPLIT_COVERS_SMALLK_DB))"""
    if not hasattr(L, "kmc_hip_smallk_tally"):
        return
    vp = C.c_void_p
    L.kmc_hip_smallk_tally.argtypes = [vp, C.c_int, vp, C.c_uint32, C.c_uint64, C.c_uint64, u64p]
    L.kmc_hip_smallk_view_device.argtypes = [vp, C.c_int, vp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint64, vp,
                                             C.POINTER(DbView), u64p, u64p]


def bind_sigstats(L):
    """the prototypes of the stage-0 statistics on a loaded library (added within ABI version 4: ask kmc_hip_split_covers(SPLIT_COVERS_SIGSTATS))"""
    if not hasattr(L, "kmc_hip_sigstats_open"):
        return
    vp = C.c_void_p
    L.kmc_hip_sigstats_open.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32]
    L.kmc_hip_sigstats_part.argtypes = [vp, C.c_int, C.c_int, C.POINTER(SplitParams), vp, C.c_uint64, u64p, u64p]
    L.kmc_hip_sigstats_read.argtypes = [vp, C.c_int, C.c_uint64, C.c_uint64, vp]
    L.kmc_hip_sigstats_close.argtypes = [vp, C.c_int]
    L.kmc_hip_sigstats_allowed.argtypes = [C.c_uint32, vp]


def _vp(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


class Context:
    """kmc_hip_ctx: one per process, `devices` = HIP ordinals."""

    def __init__(self, devices=(0,)):
        self.L = load()
        ids = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        rc = self.L.kmc_hip_init(ids, len(devices), C.byref(h))
        if rc:
            raise KmcHipError(rc, self.L.kmc_hip_last_error(None).decode())
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.kmc_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise KmcHipError(rc, self.L.kmc_hip_last_error(self.h).decode())

    # ---- derived sizes
    def out_rec_bytes(self, p: BinParams) -> int:
        return self.L.kmc_hip_out_rec_bytes(C.byref(p))

    def lut_entries(self, p: BinParams) -> int:
        return self.L.kmc_hip_lut_entries(C.byref(p))

    # ---- narrow boundary
    def sort_records(self, recs: np.ndarray, key_bytes: int, dev: int = 0) -> np.ndarray:
        """Sort (n, words) uint64 records ascending by their low key_bytes bytes; returns a sorted copy."""
        r = np.ascontiguousarray(recs, dtype=np.uint64).copy()
        if r.ndim == 1:
            r = r.reshape(-1, 1)
        self._chk(self.L.kmc_hip_sort_records(self.h, dev, _vp(r), r.shape[0], r.shape[1], key_bytes))
        return r

    # ---- full boundary
    def process_bin(self, p: BinParams, image: np.ndarray, n_rec: int, pack_bytes=None, out_capacity=None, dev: int = 0, multi: bool = False):
        """One bin through kmc_hip_process_bin — or, multi=True, through kmc_hip_process_bin_multi: the same bin over every device of the context.
        Returns (suffix_bytes ndarray, lut ndarray, stats ndarray[4])."""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        rec = self.out_rec_bytes(p)
        if out_capacity is None:
            out_capacity = ((n_rec + 1) // max(p.cutoff_min, 1)) * rec  # kb_reader.h:141-150
        out = np.zeros(max(out_capacity, 1), dtype=np.uint8)
        nl = self.lut_entries(p)
        lut = np.zeros(max(nl, 1), dtype=np.uint64)
        stats = np.zeros(4, dtype=np.uint64)
        ob = C.c_uint64()
        if pack_bytes is None:
            pb, npk = None, 0
        else:
            pack_bytes = np.ascontiguousarray(pack_bytes, dtype=np.uint64)
            pb, npk = _vp(pack_bytes), pack_bytes.size
        src = image if image.size else np.zeros(1, dtype=np.uint8)
        if multi:
            self._chk(self.L.kmc_hip_process_bin_multi(self.h, C.byref(p), _vp(src), image.size, n_rec, pb, npk, _vp(out), out_capacity, C.byref(ob), _vp(lut),
                                                       stats.ctypes.data_as(u64p)))
        else:
            self._chk(self.L.kmc_hip_process_bin(self.h, dev, C.byref(p), _vp(src), image.size, n_rec, pb, npk, _vp(out), out_capacity,
                                                 C.byref(ob), _vp(lut), stats.ctypes.data_as(u64p)))
        return out[: ob.value].copy(), lut[:nl].copy(), stats

    def process_bins_host(self, p: BinParams, bins, out_capacity=None, slot: int = 0, dev: int = 0):
        """Up to 16 bins [(image, n_rec, pack_bytes or None), ...] through ONE kmc_hip_process_bins_submit / _wait pair (the bins are sorted together
        where the key has spare bits). Returns [(suffix_bytes, lut, stats[4]), ...] in the order of the bins."""
        n = len(bins)
        rec, nl = self.out_rec_bytes(p), self.lut_entries(p)
        arr = (HostBin * max(n, 1))()
        keep, outs, luts = [], [], []
        for i, (image, n_rec, pack_bytes) in enumerate(bins):
            image = np.ascontiguousarray(image, dtype=np.uint8)
            cap = ((n_rec + 1) // max(p.cutoff_min, 1)) * rec if out_capacity is None else out_capacity
            out, lut = np.zeros(max(cap, 1), dtype=np.uint8), np.zeros(max(nl, 1), dtype=np.uint64)
            src = image if image.size else np.zeros(1, dtype=np.uint8)
            pb = None if pack_bytes is None else np.ascontiguousarray(pack_bytes, dtype=np.uint64)
            keep += [src, pb]
            outs.append(out)
            luts.append(lut)
            arr[i] = HostBin(src.ctypes.data, image.size, n_rec, None if pb is None else pb.ctypes.data, 0 if pb is None else pb.size, out.ctypes.data, cap,
                             lut.ctypes.data)
        self._chk(self.L.kmc_hip_process_bins_submit(self.h, dev, slot, C.byref(p), arr, n))
        ob, st = np.zeros(max(n, 1), dtype=np.uint64), np.zeros((max(n, 1), 4), dtype=np.uint64)
        self._chk(self.L.kmc_hip_process_bins_wait(self.h, dev, slot, ob.ctypes.data_as(u64p), st.ctypes.data_as(u64p)))
        return [(outs[i][: int(ob[i])].copy(), luts[i][:nl].copy(), st[i].copy()) for i in range(n)]

    # ---- stage-isolating test hooks
    def debug_expand(self, p: BinParams, image: np.ndarray, n_rec: int, pack_bytes: np.ndarray, dev: int = 0) -> np.ndarray:
        words = (p.kmer_len + 31) // 32
        out = np.zeros((n_rec, words), dtype=np.uint64)
        pack_bytes = np.ascontiguousarray(pack_bytes, dtype=np.uint64)
        self._chk(self.L.kmc_hip_debug_expand(self.h, dev, C.byref(p), _vp(image), image.size, n_rec, _vp(pack_bytes), pack_bytes.size, _vp(out)))
        return out

    def debug_compact(self, p: BinParams, sorted_recs: np.ndarray, out_capacity=None, dev: int = 0):
        r = np.ascontiguousarray(sorted_recs, dtype=np.uint64)
        n = r.shape[0]
        rec = self.out_rec_bytes(p)
        if out_capacity is None:
            out_capacity = (n + 1) * rec
        out = np.zeros(max(out_capacity, 1), dtype=np.uint8)
        nl = self.lut_entries(p)
        lut = np.zeros(max(nl, 1), dtype=np.uint64)
        stats = np.zeros(4, dtype=np.uint64)
        ob = C.c_uint64()
        self._chk(self.L.kmc_hip_debug_compact(self.h, dev, C.byref(p), _vp(r), n, _vp(out), out_capacity, C.byref(ob), _vp(lut),
                                               stats.ctypes.data_as(u64p)))
        return out[: ob.value].copy(), lut[:nl].copy(), stats

    def debug_split_reads(self, codes: np.ndarray, k: int, sig_len: int = 9, dev: int = 0):
        """stage-1 test hook: code stream (int8, negative = N / read boundary) -> (sig per position, sk_pos, sk_len, sk_sig)"""
        codes = np.ascontiguousarray(codes, dtype=np.int8)
        n = codes.size
        sig = np.zeros(max(n, 1), dtype=np.uint32)
        cap = n + 8
        pos = np.zeros(cap, dtype=np.uint64)
        ln = np.zeros(cap, dtype=np.uint32)
        sg = np.zeros(cap, dtype=np.uint32)
        nsk = C.c_uint64()
        self._chk(self.L.kmc_hip_debug_split_reads(self.h, dev, _vp(codes), n, k, sig_len, _vp(sig), _vp(pos), _vp(ln), _vp(sg), cap, C.byref(nsk)))
        j = nsk.value
        return sig[:n], pos[:j].copy(), ln[:j].copy(), sg[:j].copy()

    def split_reads_device(self, d_codes: int, n: int, k: int, sig_len: int, d_sig_to_bin: int, n_bins: int, dev: int = 0):
        """stage 1 on the device (groundwork, include/kmc_hip.h): device code stream -> bins in HBM. Returns dict(d_bins, d_pack_start, base, bytes,
        superkmers, kmers, pack_base); the caller frees d_bins / d_pack_start with free()."""
        base = np.zeros(n_bins + 1, dtype=np.uint64)
        pbase = np.zeros(n_bins + 1, dtype=np.uint64)
        by, sk, km = (np.zeros(n_bins, dtype=np.uint64) for _ in range(3))
        plan = C.c_void_p()
        self.L.kmc_hip_split_reads_free.restype = None
        self._chk(self.L.kmc_hip_split_reads_plan(self.h, dev, C.c_void_p(d_codes), C.c_uint64(n), C.c_uint32(k), C.c_uint32(sig_len), C.c_void_p(d_sig_to_bin),
                                                  C.c_uint32(n_bins), C.byref(plan), _vp(base), _vp(by), _vp(sk), _vp(km), _vp(pbase)))
        d_bins = d_ps = None
        try:
            d_bins = self.malloc(int(base[n_bins]), dev)
            d_ps = self.malloc(int(pbase[n_bins]) * 8, dev)
            self._chk(self.L.kmc_hip_split_reads_emit(self.h, plan, C.c_void_p(d_bins), C.c_void_p(d_ps)))
        except Exception:
            for q in (d_bins, d_ps):
                if q:
                    self.free(q, dev)
            raise
        finally:
            self.L.kmc_hip_split_reads_free(self.h, plan)
        return dict(d_bins=d_bins, d_pack_start=d_ps, base=base, bytes=by, superkmers=sk, kmers=km, pack_base=pbase)

    # ---- device memory helpers
    def malloc(self, nbytes: int, dev: int = 0) -> int:
        p = C.c_void_p()
        self._chk(self.L.kmc_hip_malloc(self.h, dev, nbytes, C.byref(p)))
        return p.value

    def free(self, dptr: int, dev: int = 0):
        self._chk(self.L.kmc_hip_free(self.h, dev, C.c_void_p(dptr)))

    def h2d(self, dptr: int, a: np.ndarray, dev: int = 0):
        a = np.ascontiguousarray(a)
        self._chk(self.L.kmc_hip_memcpy_h2d(self.h, dev, C.c_void_p(dptr), _vp(a), a.nbytes))

    def d2h(self, a: np.ndarray, dptr: int, dev: int = 0):
        self._chk(self.L.kmc_hip_memcpy_d2h(self.h, dev, _vp(a), C.c_void_p(dptr), a.nbytes))

    def synchronize(self, dev: int = 0):
        self._chk(self.L.kmc_hip_synchronize(self.h, dev))

    def process_bin_device(self, p: BinParams, d_image: int, size: int, n_rec: int, d_pack_start: int, n_packs: int, d_out: int,
                           out_capacity: int, d_out_bytes: int, d_lut: int, d_stats: int, sync: bool = True, dev: int = 0):
        self._chk(self.L.kmc_hip_process_bin_device(self.h, dev, C.byref(p), C.c_void_p(d_image), size, n_rec, C.c_void_p(d_pack_start),
                                                    n_packs, C.c_void_p(d_out), out_capacity, C.c_void_p(d_out_bytes),
                                                    C.c_void_p(d_lut), C.c_void_p(d_stats), 1 if sync else 0))

    def sort_records_device(self, d_recs: int, d_tmp: int, n: int, words: int, key_bytes: int, dev: int = 0) -> int:
        res = C.c_void_p()
        self._chk(self.L.kmc_hip_sort_records_device(self.h, dev, C.c_void_p(d_recs), C.c_void_p(d_tmp), n, words, key_bytes, C.byref(res)))
        return res.value

    def last_timings(self, dev: int = 0):
        ms = (C.c_float * 6)()
        self._chk(self.L.kmc_hip_last_timings(self.h, dev, ms))
        return dict(zip(("index", "expand", "hist", "scatter", "compact", "total"), [float(x) for x in ms]))

    def scatter_totals(self, reset: bool = True, dev: int = 0):
        """(launches, summed ms, records moved) of all k_onesweep launches completed on `dev` since the last reset."""
        n, t, k = C.c_uint64(), C.c_double(), C.c_uint64()
        self._chk(self.L.kmc_hip_scatter_totals(self.h, dev, 1 if reset else 0, C.byref(n), C.byref(t), C.byref(k)))
        return n.value, t.value, k.value

    def set_hybrid(self, mode: int) -> int:
        """process-wide sort selection (see include/kmc_hip.h kmc_hip_set_hybrid); returns the previous mode"""
        self.L.kmc_hip_set_hybrid.restype = C.c_int
        return int(self.L.kmc_hip_set_hybrid(C.c_int(mode)))

    def local_sort_totals(self, reset: bool = True, dev: int = 0):
        """dict(launches, ms, records) of the LDS half of the hybrid sort on `dev` since the last reset + process-wide hybrid / redo group counts."""
        n, t, k, h, r = C.c_uint64(), C.c_double(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(self.L.kmc_hip_local_sort_totals(self.h, dev, 1 if reset else 0, C.byref(n), C.byref(t), C.byref(k), C.byref(h), C.byref(r)))
        return dict(launches=n.value, ms=t.value, records=k.value, hybrid_groups=h.value, redo_groups=r.value)

    def path_counters(self, dev: int = 0):
        """group counts by path since the last set_hybrid (process-wide) + the tiles / records k_giant_tiles took on `dev` since the context was made:
        dict(rank_count, rank_compact, bucket_count, lsd, giant_tiles, giant_records, indirect); `indirect`: the groups of rank_count whose HBM passes moved
        (key top, record number) pairs instead of records (three words and more)"""
        c = (C.c_uint64 * 8)()
        self._chk(self.L.kmc_hip_path_counters(self.h, dev, c))
        return dict(rank_count=c[0], rank_compact=c[1], bucket_count=c[2], lsd=c[3], giant_tiles=c[4], giant_records=c[5], indirect=c[6])

    def process_bins_device(self, p: BinParams, descs, n_streams: int = 0, dev: int = 0):
        """Enqueue many device-resident bins (ctypes array of BinDesc); returns after enqueueing — call synchronize()."""
        self._chk(self.L.kmc_hip_process_bins_device(self.h, dev, C.byref(p), descs, len(descs), n_streams))

    def order_database_device(self, p: BinParams, descs, out_lut_prefix_len: int, d_out: int, out_capacity: int, d_lut_out: int, dev: int = 0) -> int:
        """All counted k-mers of the bins (device-resident outputs of process_bins_device) as ONE ascending sequence; returns the number of records."""
        n = C.c_uint64()
        self._chk(self.L.kmc_hip_order_database_device(self.h, dev, C.byref(p), descs, len(descs), out_lut_prefix_len, d_out, out_capacity, d_lut_out, C.byref(n)))
        return n.value

    def db_set_op_device(self, kmer_len: int, a: DbView, b: DbView, op: DbOp, d_out: int, out_capacity: int, d_lut_out: int, dev: int = 0):
        """One `kmc_tools simple` operation between two device-resident KMC1 bodies (kmc_hip_db_set_op_device); returns (records written, dict of the six tallies)."""
        if not hasattr(self.L, "kmc_hip_db_set_op_device"):
            raise KmcHipError(-1, f"{lib_path()} has no kmc_hip_db_set_op_device")
        n = C.c_uint64()
        st = (C.c_uint64 * 6)()
        self._chk(self.L.kmc_hip_db_set_op_device(self.h, dev, kmer_len, C.byref(a), C.byref(b), C.byref(op), d_out, out_capacity, d_lut_out, C.byref(n), st))
        return n.value, dict(zip(DB_STATS, (int(x) for x in st)))

    def db_query_reads_device(self, db: DbView, kmer_len: int, both_strands: bool, d_seq: int, n_bytes: int, d_read_off: int, n_reads: int, threshold: int, d_counters: int,
                              d_n_valid: int = 0, d_trim_len: int = 0, d_masked: int = 0, dev: int = 0) -> dict:
        """The reads in d_seq against a device-resident KMC1 body (kmc_hip_db_query_reads_device): fills d_counters[n_bytes] and, where given, d_n_valid[n_reads],
        d_trim_len[n_reads], d_masked[n_bytes]; returns the dict of the four tallies."""
        if not hasattr(self.L, "kmc_hip_db_query_reads_device"):
            raise KmcHipError(-1, f"{lib_path()} has no kmc_hip_db_query_reads_device")
        st = (C.c_uint64 * 4)()
        self._chk(self.L.kmc_hip_db_query_reads_device(self.h, dev, C.byref(db), kmer_len, 1 if both_strands else 0, d_seq or None, n_bytes, d_read_off or None, n_reads, threshold,
                                                       d_counters or None, d_n_valid or None, d_trim_len or None, d_masked or None, st))
        return dict(zip(DBQ_STATS, (int(x) for x in st)))

    def _need(self, name):
        if not hasattr(self.L, name):
            raise KmcHipError(-1, f"{lib_path()} has no {name}")

    def db_reduce_device(self, kmer_len: int, db: DbView, cutoff_min: int, cutoff_max: int, counter_max: int, counter_value: int, out_lut_prefix_len: int, d_out: int,
                         out_capacity: int, d_lut_out: int, dev: int = 0):
        """A database output of `kmc_tools transform` (reduce, compact, set_counts, sort of an ordered body) from a device-resident KMC1 body (kmc_hip_db_reduce_device);
        returns (records written, dict of the four tallies)."""
        self._need("kmc_hip_db_reduce_device")
        n = C.c_uint64()
        st = (C.c_uint64 * 4)()
        self._chk(self.L.kmc_hip_db_reduce_device(self.h, dev, kmer_len, C.byref(db), cutoff_min, cutoff_max, counter_max, counter_value, out_lut_prefix_len, d_out or None, out_capacity,
                                                  d_lut_out or None, C.byref(n), st))
        return n.value, dict(zip(DBT_STATS, (int(x) for x in st)))

    def db_histogram_device(self, kmer_len: int, db: DbView, n_lut_segments: int, cutoff_min: int, cutoff_max: int, d_hist: int, dev: int = 0) -> dict:
        """The counters of a device-resident body counted into d_hist[cutoff_max - cutoff_min + 1] (kmc_hip_db_histogram_device); returns the dict of the three tallies."""
        self._need("kmc_hip_db_histogram_device")
        st = (C.c_uint64 * 3)()
        self._chk(self.L.kmc_hip_db_histogram_device(self.h, dev, kmer_len, C.byref(db), n_lut_segments, cutoff_min, cutoff_max, d_hist or None, st))
        return dict(zip(DBH_STATS, (int(x) for x in st)))

    def db_dump_device(self, kmer_len: int, db: DbView, n_lut_segments: int, first: int, count: int, cutoff_min: int, cutoff_max: int, counter_max: int, d_text: int,
                       text_capacity: int, dev: int = 0):
        """Records [first, first + count) of a device-resident body as the text of `kmc_tools transform dump` (kmc_hip_db_dump_device); returns (bytes written, dict of the
        four tallies)."""
        self._need("kmc_hip_db_dump_device")
        n = C.c_uint64()
        st = (C.c_uint64 * 4)()
        self._chk(self.L.kmc_hip_db_dump_device(self.h, dev, kmer_len, C.byref(db), n_lut_segments, first, count, cutoff_min, cutoff_max, counter_max, d_text or None, text_capacity,
                                                C.byref(n), st))
        return n.value, dict(zip(DBT_STATS, (int(x) for x in st)))

    def db_compare_device(self, kmer_len: int, a: DbView, b: DbView, dev: int = 0) -> dict:
        """`kmc_tools compare` between two device-resident KMC1 bodies (kmc_hip_db_compare_device); returns the dict of DBC_RESULT (kind: an index into DBC_KINDS)."""
        self._need("kmc_hip_db_compare_device")
        res = (C.c_uint64 * 8)()
        self._chk(self.L.kmc_hip_db_compare_device(self.h, dev, kmer_len, C.byref(a), C.byref(b), res))
        return dict(zip(DBC_RESULT, (int(x) for x in res)))

    def db_expr_device(self, kmer_len: int, views, steps, out: DbOp, d_out: int, out_capacity: int, d_lut_out: int, dev: int = 0):
        """One `kmc_tools complex` expression over device-resident KMC1 bodies (kmc_hip_db_expr_device). views: DbView's; steps: the postfix program as (kind, arg) pairs
        (expr_steps makes them); out: a DbOp whose op and counter_op are ignored. Returns (records written, dict of DBX_STATS)."""
        self._need("kmc_hip_db_expr_device")
        va, sa = (DbView * max(len(views), 1))(*views), (DbExprStep * max(len(steps), 1))(*[DbExprStep(*s) for s in steps])
        n, st = C.c_uint64(), (C.c_uint64 * 5)()
        self._chk(self.L.kmc_hip_db_expr_device(self.h, dev, kmer_len, va, len(views), sa, len(steps), C.byref(out), d_out, out_capacity, d_lut_out, C.byref(n), st))
        return n.value, dict(zip(DBX_STATS, (int(x) for x in st)))

    def kff_import_device(self, kmer_len: int, data_size: int, d_kff: int, section_n_recs, ordered: bool, out_lut_prefix_len: int, d_out: int, out_capacity: int,
                          d_lut_out: int, dev: int = 0) -> int:
        """The records of a KFF file's raw sections (d_kff: back to back; section_n_recs: records per section) as a database body (kmc_hip_kff_import_device): ordered, one
        ascending body under a KMC1 LUT; otherwise the body in file order under the segmented LUT of len(section_n_recs) x 4^p + 1 entries. Returns the number of records."""
        self._need("kmc_hip_kff_import_device")
        sec = (C.c_uint64 * max(len(section_n_recs), 1))(*[int(x) for x in section_n_recs])
        n = C.c_uint64()
        self._chk(self.L.kmc_hip_kff_import_device(self.h, dev, kmer_len, data_size, d_kff or None, sec, len(section_n_recs), 1 if ordered else 0, out_lut_prefix_len, d_out or None,
                                                   out_capacity, d_lut_out or None, C.byref(n)))
        return n.value

    def db_kff_export_device(self, kmer_len: int, db: DbView, n_lut_segments: int, first: int, count: int, data_size: int, d_kff: int, kff_capacity: int, dev: int = 0) -> int:
        """Records [first, first + count) of a device-resident body framed as KFF records of ceil(kmer_len / 4) + data_size bytes in d_kff (kmc_hip_db_kff_export_device);
        n_lut_segments as for db_dump_device. The view's cutoffs are not read. Returns the bytes written."""
        self._need("kmc_hip_db_kff_export_device")
        self._chk(self.L.kmc_hip_db_kff_export_device(self.h, dev, kmer_len, C.byref(db), n_lut_segments, first, count, data_size, d_kff or None, kff_capacity))
        return count * ((kmer_len + 3) // 4 + data_size)

    def debug_gather_segments(self, d_src: int, d_dst: int, table: np.ndarray, dev: int = 0):
        """test hook: k_cnt_gather on a table of (source offset, destination offset, bytes) triples over two device buffers"""
        bind_count(self.L)
        t = np.ascontiguousarray(table, dtype=np.uint64).reshape(-1, 3)
        self._chk(self.L.kmc_hip_debug_gather_segments(self.h, dev, C.c_void_p(d_src), C.c_void_p(d_dst), _vp(t) if t.size else None, t.shape[0]))

    def host_alloc(self, nbytes: int) -> np.ndarray:
        """Pinned host memory as a uint8 array (free with host_free(arr))."""
        p = C.c_void_p()
        self._chk(self.L.kmc_hip_host_alloc(self.h, nbytes, C.byref(p)))
        a = np.ctypeslib.as_array(C.cast(p, u8p), shape=(max(nbytes, 1),))
        return a

    def host_free(self, arr: np.ndarray):
        self._chk(self.L.kmc_hip_host_free(self.h, C.c_void_p(arr.ctypes.data)))

    def device_count(self) -> int:
        return self.L.kmc_hip_device_count()

    def allreduce_stats(self, per_dev: np.ndarray) -> np.ndarray:
        a = np.ascontiguousarray(per_dev, dtype=np.uint64).copy()
        self._chk(self.L.kmc_hip_allreduce_stats(self.h, a.ctypes.data_as(u64p)))
        return a


class CountSession:
    """kmc_hip_count: a reads file part by part -> one ordered database body on the device (include/kmc_hip.h). ctx: a Context, or anything with its L, h and _chk.
    k, signature length, number of bins and strands are fixed here; the signature map (4^m + 1 int32) is uploaded with kmc_hip_split_set_map."""

    def __init__(self, ctx, k: int, signature_len: int, n_bins: int, both_strands: bool, sig_map: np.ndarray, dev: int = 0):
        self.ctx, self.dev, self.h = ctx, dev, None
        if not hasattr(ctx.L, "kmc_hip_count_open"):
            raise KmcHipError(-1, f"{lib_path()} has no kmc_hip_count_open")
        bind_count(ctx.L)
        self.fixed = (k, signature_len, n_bins, 1 if both_strands else 0)
        sig_map = np.ascontiguousarray(sig_map, dtype=np.int32)
        assert sig_map.size == (1 << (2 * signature_len)) + 1
        ctx._chk(ctx.L.kmc_hip_split_set_map(ctx.h, dev, _vp(sig_map), signature_len))
        h = C.c_void_p()
        ctx._chk(ctx.L.kmc_hip_count_open(ctx.h, dev, C.byref(self.split_params()), C.byref(h)))
        self.h = h

    def split_params(self, file_type: int = 1, line_cap: int = SPLIT_LINE_CAP, part_kind: int = 0, flags: int = 0, **other) -> SplitParams:
        """the session's parameters with a part's own; **other overrides fields (tests)"""
        k, m, n_bins, both = self.fixed
        p = SplitParams(k, m, n_bins, 0, both, file_type, line_cap, part_kind, flags)
        for name, v in other.items():
            setattr(p, name, v)
        return p

    def part_rc(self, text, p: SplitParams, slot: int = 0):
        """one part; -> (return code, reads): the code is 0, UNCOVERED or negative, nothing is raised"""
        t = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)
        n = C.c_uint64(0)
        rc = self.ctx.L.kmc_hip_count_part(self.ctx.h, self.h, slot, C.byref(p), _vp(t) if t.size else None, t.size, C.byref(n))
        return rc, n.value

    def part(self, text, p: SplitParams, slot: int = 0) -> int:
        """one part; returns its reads. KMC_HIP_UNCOVERED raises like an error: the session is as it was"""
        rc, n = self.part_rc(text, p, slot)
        if rc == UNCOVERED:
            raise KmcHipError(rc, "KMC_HIP_UNCOVERED: the part's text is malformed in a way the device splitter does not reproduce (blank lines, a quality line of another "
                                  "length than its sequence, control characters)")
        self.ctx._chk(rc)
        return n

    def finish(self, bp: BinParams):
        """-> (stats[4] in KMC_HIP_STAT_* order, totals[4] = reads, super-k-mers, k-mers, bytes of bin records, records kept)"""
        st, tot, n = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64), C.c_uint64(0)
        self.ctx._chk(self.ctx.L.kmc_hip_count_finish(self.ctx.h, self.h, C.byref(bp), st.ctypes.data_as(u64p), tot.ctypes.data_as(u64p), C.byref(n)))
        return st, tot, n.value

    def order(self, out_lut_prefix_len: int) -> DbView:
        """the ordered body as a view; its memory is the session's and lives until the next order() or close()"""
        v = DbView()
        self.ctx._chk(self.ctx.L.kmc_hip_count_order(self.ctx.h, self.h, out_lut_prefix_len, C.byref(v)))
        return v

    def info(self) -> dict:
        a = np.zeros(6, dtype=np.uint64)
        self.ctx._chk(self.ctx.L.kmc_hip_count_info(self.ctx.h, self.h, a.ctypes.data_as(u64p)))
        return dict(zip(("n_parts", "n_chunks", "n_segments", "n_batches", "largest_bin", "bins_in_use"), (int(x) for x in a)))

    def timings(self) -> dict:
        """seconds of the last finish() and order(): dict(layout, gather, stage2, order); gather by HIP events around k_cnt_gather, the others wall clock"""
        t = (C.c_double * 4)()
        self.ctx._chk(self.ctx.L.kmc_hip_count_timings(self.ctx.h, self.h, t))
        return dict(zip(("layout", "gather", "stage2", "order"), (float(x) for x in t)))

    def close(self):
        if self.h:
            self.ctx.L.kmc_hip_count_close(self.ctx.h, self.h)
            self.h = None


def allowed_signatures(signature_len: int, L=None) -> np.ndarray:
    """bool[4^m + 1]: the m-mers that can be a signature (CMmer::is_allowed, as the kernels compute it); the last entry, the special signature's, is False.
    L: a loaded library (a Context's L); by default the in-tree one"""
    L = L or load()
    bind_sigstats(L)
    out = np.zeros((1 << (2 * signature_len)) + 1, dtype=np.uint8)
    rc = L.kmc_hip_sigstats_allowed(signature_len, _vp(out))
    if rc:
        raise KmcHipError(rc, L.kmc_hip_last_error(None).decode())
    return out.astype(bool)


class SigStats:
    """kmc_hip_sigstats: the stage-0 statistics of one (k, signature length) on a device — stats[s] = the k-mer windows whose signature is s, 4^m + 1 uint32
    (include/kmc_hip.h). ctx: a Context, or anything with its L, h and _chk."""

    def __init__(self, ctx, k: int, signature_len: int, dev: int = 0):
        self.ctx, self.dev, self.k, self.m, self.open = ctx, dev, k, signature_len, False
        if not hasattr(ctx.L, "kmc_hip_sigstats_open") or ctx.L.kmc_hip_split_covers(SPLIT_COVERS_SIGSTATS) != 1:
            raise KmcHipError(-1, f"{lib_path()} has no kmc_hip_sigstats_open")
        bind_sigstats(ctx.L)
        ctx._chk(ctx.L.kmc_hip_sigstats_open(ctx.h, dev, k, signature_len))
        self.open = True

    @property
    def entries(self) -> int:
        return (1 << (2 * self.m)) + 1

    def part_rc(self, text, file_type: int = 1, line_cap: int = SPLIT_LINE_CAP, part_kind: int = 0, flags: int = 0, slot: int = 0):
        """one part; -> (return code, reads, windows added): the code is 0, UNCOVERED or negative, nothing is raised"""
        p = SplitParams(self.k, self.m, 0, 0, 0, file_type, line_cap, part_kind, flags)
        t = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)
        n_reads, n_kmers = C.c_uint64(0), C.c_uint64(0)
        rc = self.ctx.L.kmc_hip_sigstats_part(self.ctx.h, self.dev, slot, C.byref(p), _vp(t) if t.size else None, t.size, C.byref(n_reads), C.byref(n_kmers))
        return rc, n_reads.value, n_kmers.value

    def part(self, text, **kw):
        """one part; -> (reads, windows added). KMC_HIP_UNCOVERED raises like an error: the statistics are as they were"""
        rc, n_reads, n_kmers = self.part_rc(text, **kw)
        if rc == UNCOVERED:
            raise KmcHipError(rc, "KMC_HIP_UNCOVERED: the part's text is malformed in a way the device splitter does not reproduce")
        self.ctx._chk(rc)
        return n_reads, n_kmers

    def read(self, first: int = 0, count: int = None) -> np.ndarray:
        count = self.entries - first if count is None else count
        out = np.zeros(max(count, 1), dtype=np.uint32)
        self.ctx._chk(self.ctx.L.kmc_hip_sigstats_read(self.ctx.h, self.dev, first, count, _vp(out)))
        return out[:count]

    def close(self):
        if self.open:
            self.ctx.L.kmc_hip_sigstats_close(self.ctx.h, self.dev)
            self.open = False


SPLIT_COVERS_SMALLK_DB = 0x109  # KMC_HIP_SPLIT_COVERS_SMALLK_DB
SMALLK_STATS = ("n_unique", "n_cutoff_min", "n_cutoff_max", "n_kept")  # stats[] of kmc_hip_smallk_tally and kmc_hip_smallk_view_device, in order
SMALLK_KMC1, SMALLK_KFF = 0, 1  # the framings of kmc_hip_smallk_view_device


def counter_size(cutoff_max: int, counter_max: int, L=None) -> int:
    return int((L or load()).kmc_hip_counter_size(cutoff_max, counter_max))


class SmallK:
    """The small-k table (k <= 13) of one device: reads in part by part (kmc_hip_smallk_open / _part), then the table tallied and framed as a database body or as KFF
    records where it lies (kmc_hip_smallk_tally / _view_device), or read back (kmc_hip_smallk_read). ctx: a Context, or anything with its L, h, _chk, malloc and free. view() owns
    the body and the LUT it makes until the next view() or close()."""

    def __init__(self, ctx, k: int, both_strands: bool, dev: int = 0):
        self.ctx, self.dev, self.k, self.both, self.open, self._bufs = ctx, dev, k, 1 if both_strands else 0, False, []
        if not hasattr(ctx.L, "kmc_hip_smallk_tally") or ctx.L.kmc_hip_split_covers(SPLIT_COVERS_SMALLK_DB) != 1:
            raise KmcHipError(-1, f"{lib_path()} has no kmc_hip_smallk_tally")
        bind_smallk_db(ctx.L)
        ctx._chk(ctx.L.kmc_hip_smallk_open(ctx.h, dev, k, self.both))
        self.open = True

    @property
    def entries(self) -> int:
        return 1 << (2 * self.k)

    def part_rc(self, text, file_type: int = 1, line_cap: int = SPLIT_LINE_CAP, part_kind: int = 0, flags: int = 0, slot: int = 0):
        """one part; -> (return code, reads, k-mers counted): the code is 0, UNCOVERED or negative, nothing is raised"""
        p = SplitParams(self.k, 0, 0, 0, self.both, file_type, line_cap, part_kind, flags)
        t = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)
        n_reads, n_kmers = C.c_uint64(0), C.c_uint64(0)
        rc = self.ctx.L.kmc_hip_smallk_part(self.ctx.h, self.dev, slot, C.byref(p), _vp(t) if t.size else None, t.size, C.byref(n_reads), C.byref(n_kmers))
        return rc, n_reads.value, n_kmers.value

    def part(self, text, **kw):
        """one part; -> (reads, k-mers counted). KMC_HIP_UNCOVERED raises like an error: the table is as it was"""
        rc, n_reads, n_kmers = self.part_rc(text, **kw)
        if rc == UNCOVERED:
            raise KmcHipError(rc, "KMC_HIP_UNCOVERED: the part's text is malformed in a way the device splitter does not reproduce")
        self.ctx._chk(rc)
        return n_reads, n_kmers

    def read(self, first: int = 0, count: int = None) -> np.ndarray:
        count = self.entries - first if count is None else count
        out = np.zeros(max(count, 1), dtype=np.uint64)
        self.ctx._chk(self.ctx.L.kmc_hip_smallk_read(self.ctx.h, self.dev, first, count, _vp(out)))
        return out[:count]

    def tally(self, cutoff_min: int, cutoff_max: int, d_table: int = 0) -> dict:
        """dict of SMALLK_STATS over the open table (or over d_table: 4^k uint64 on the device)"""
        st = np.zeros(4, dtype=np.uint64)
        self.ctx._chk(self.ctx.L.kmc_hip_smallk_tally(self.ctx.h, self.dev, d_table or None, self.k, cutoff_min, cutoff_max, st.ctypes.data_as(u64p)))
        return dict(zip(SMALLK_STATS, (int(x) for x in st)))

    def _malloc(self, nbytes: int) -> int:
        d = self.ctx.malloc(nbytes, self.dev) if self.dev else self.ctx.malloc(nbytes)
        self._bufs.append(d)
        return d

    def _free(self):
        for b in self._bufs:
            self.ctx.free(b, self.dev) if self.dev else self.ctx.free(b)
        self._bufs = []

    def view(self, cutoff_min: int, cutoff_max: int, counter_max: int, lut_prefix_len: int = 0, framing: int = SMALLK_KMC1, data_size: int = 0, d_table: int = 0):
        """the table as a body on the device, sized by a tally. KMC1 -> (DbView, stats dict): the body and its LUT of 4^lut_prefix_len entries; KFF -> ((device pointer,
        bytes), stats dict): records of ceil(k / 4) + data_size bytes. The memory is this object's until the next view() or close()."""
        self._free()
        kept = self.tally(cutoff_min, cutoff_max, d_table)["n_kept"]
        cs = counter_size(cutoff_max, counter_max, self.ctx.L)
        rb = ((self.k + 3) // 4 + data_size) if framing == SMALLK_KFF else (max(self.k - lut_prefix_len, 0) // 4 + cs)
        cap = kept * rb
        d_out = self._malloc(cap + 16)
        d_lut = self._malloc(8 << (2 * min(max(lut_prefix_len, 0), 13))) if framing == SMALLK_KMC1 else 0
        v, n, st = DbView(), C.c_uint64(0), np.zeros(4, dtype=np.uint64)
        self.ctx._chk(self.ctx.L.kmc_hip_smallk_view_device(self.ctx.h, self.dev, d_table or None, self.k, self.both, cutoff_min, cutoff_max, counter_max, framing, lut_prefix_len,
                                                            data_size, d_out, cap, d_lut or None, C.byref(v), C.byref(n), st.ctypes.data_as(u64p)))
        stats = dict(zip(SMALLK_STATS, (int(x) for x in st)))
        return ((d_out, n.value * rb) if framing == SMALLK_KFF else v), stats

    def close(self):
        self._free()
        if self.open:
            self.ctx.L.kmc_hip_smallk_close(self.ctx.h, self.dev)
            self.open = False


# ---- BGZF input (BAM, bgzipped FASTA / FASTQ): the member table on the host, the members inflated on the device
SPLIT_COVERS_BGZF = 0x10B  # KMC_HIP_SPLIT_COVERS_BGZF: kmc_hip_bgzf_scan / _inflate_device / _inflate, kmc_hip_bam_whole_records (0x10A stays unknown)
BGZF_NONE = 0xFFFFFFFF  # KMC_HIP_BGZF_NONE
BGZF_MEMBER = np.dtype([("src_off", "<u8"), ("dst_off", "<u8"), ("comp_len", "<u4"), ("isize", "<u4"), ("crc", "<u4"), ("reserved", "<u4")])  # struct kmc_hip_bgzf_member
BGZF_REASONS = ("", "btype", "stored", "codeset", "no_eob", "repeat", "symbol", "distance", "out_short", "out_long", "in_left", "in_short", "crc", "table")  # member_errors values


def bind_bgzf(L):
    """the prototypes of the BGZF entries on a loaded library (added within ABI version 4: ask kmc_hip_split_covers(SPLIT_COVERS_BGZF))"""
    if not hasattr(L, "kmc_hip_bgzf_scan"):
        return
    vp = C.c_void_p
    L.kmc_hip_last_error.argtypes = [vp]
    L.kmc_hip_last_error.restype = C.c_char_p
    L.kmc_hip_bgzf_scan.argtypes = [vp, C.c_uint64, C.c_uint64, vp, C.c_uint64, u64p, u64p, u64p]
    L.kmc_hip_bgzf_inflate_device.argtypes = [vp, C.c_int, C.c_int, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint32), vp]
    L.kmc_hip_bgzf_inflate.argtypes = [vp, C.c_int, C.c_int, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint32), vp]
    L.kmc_hip_bgzf_last_ms.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_float)]
    L.kmc_hip_bam_whole_records.argtypes = [vp, C.c_uint64, u64p, u64p]


class BgzfError(KmcHipError):
    """KMC_HIP_ECORRUPT of an inflate call: .first_bad the smallest failing member, .member_errors the reason's number per member, .out what the other members wrote"""

    def __init__(self, code, msg, first_bad, member_errors, out):
        super().__init__(code, msg)
        self.first_bad, self.member_errors, self.out = first_bad, member_errors, out


def _bgzf_lib(L):
    L = L or load()
    if not hasattr(L, "kmc_hip_bgzf_scan"):
        raise KmcHipError(-1, f"{lib_path()} has no kmc_hip_bgzf_scan")
    bind_bgzf(L)
    return L


def _u8(a) -> np.ndarray:
    return np.frombuffer(a, dtype=np.uint8) if isinstance(a, (bytes, bytearray, memoryview)) else np.ascontiguousarray(a, dtype=np.uint8)


def bgzf_scan(src, max_out_bytes: int = 1 << 62, cap: int = None, L=None):
    """kmc_hip_bgzf_scan -> (members: BGZF_MEMBER array, bytes of src the members take, inflated bytes). Host only."""
    L = _bgzf_lib(L)
    s = _u8(src)
    cap = s.size // 26 + 1 if cap is None else cap  # a member is at least 26 bytes
    members = np.zeros(max(cap, 1), dtype=BGZF_MEMBER)
    n, used, out = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = L.kmc_hip_bgzf_scan(_vp(s) if s.size else None, s.size, max_out_bytes, _vp(members), cap, C.byref(n), C.byref(used), C.byref(out))
    if rc:
        raise KmcHipError(rc, L.kmc_hip_last_error(None).decode())
    return members[:n.value], used.value, out.value


def bgzf_inflate(ctx, src, members: np.ndarray, dst_capacity: int = None, dev: int = 0, slot: int = 0) -> np.ndarray:
    """kmc_hip_bgzf_inflate: the members of the table out of src (host bytes) -> the inflated bytes (uint8 array of the table's total, or of dst_capacity).
    ctx: a Context, or anything with its L and h. A refused member raises BgzfError."""
    L = _bgzf_lib(ctx.L)
    s, members = _u8(src), np.ascontiguousarray(members, dtype=BGZF_MEMBER)
    total = int(members["dst_off"][-1] + members["isize"][-1]) if members.size else 0
    cap = total if dst_capacity is None else dst_capacity
    out, errs, bad = np.zeros(max(cap, 1), dtype=np.uint8), np.zeros(max(members.size, 1), dtype=np.uint32), C.c_uint32(BGZF_NONE)
    rc = L.kmc_hip_bgzf_inflate(ctx.h, dev, slot, _vp(s) if s.size else None, s.size, _vp(members) if members.size else None, members.size, _vp(out), cap, C.byref(bad), _vp(errs))
    if rc:
        msg = L.kmc_hip_last_error(ctx.h).decode()
        if bad.value != BGZF_NONE:
            raise BgzfError(rc, msg, bad.value, errs[:members.size], out[:cap])
        raise KmcHipError(rc, msg)
    return out[:cap]


def bgzf_inflate_device(ctx, d_src: int, src_size: int, members: np.ndarray, d_dst: int, dst_capacity: int, dev: int = 0, slot: int = 0) -> float:
    """kmc_hip_bgzf_inflate_device on device pointers; -> the kernel's milliseconds (HIP events). A refused member raises BgzfError (out=None)."""
    L = _bgzf_lib(ctx.L)
    members = np.ascontiguousarray(members, dtype=BGZF_MEMBER)
    errs, bad, ms = np.zeros(max(members.size, 1), dtype=np.uint32), C.c_uint32(BGZF_NONE), C.c_float(0)
    rc = L.kmc_hip_bgzf_inflate_device(ctx.h, dev, slot, d_src or None, src_size, _vp(members) if members.size else None, members.size, d_dst or None, dst_capacity, C.byref(bad), _vp(errs))
    if rc:
        msg = L.kmc_hip_last_error(ctx.h).decode()
        if bad.value != BGZF_NONE:
            raise BgzfError(rc, msg, bad.value, errs[:members.size], None)
        raise KmcHipError(rc, msg)
    L.kmc_hip_bgzf_last_ms(ctx.h, dev, slot, C.byref(ms))
    return float(ms.value)


def bam_whole_records(buf, L=None):
    """kmc_hip_bam_whole_records -> (bytes of buf that are whole BAM alignment records, how many records). Host only."""
    L = _bgzf_lib(L)
    b = _u8(buf)
    n_bytes, n_recs = C.c_uint64(0), C.c_uint64(0)
    rc = L.kmc_hip_bam_whole_records(_vp(b) if b.size else None, b.size, C.byref(n_bytes), C.byref(n_recs))
    if rc:
        raise KmcHipError(rc, L.kmc_hip_last_error(None).decode())
    return n_bytes.value, n_recs.value


# ---- synthetic stage-2 inputs (libkmc_synth.so)
_SYN = None


def _syn():
    global _SYN
    if _SYN is None:
        p = _build.LIB_SYNTH
        if not os.path.exists(p):
            _build.build_synth()
        _SYN = C.CDLL(p)
        _SYN.kmc_synth_bins_range.restype = C.c_void_p
        _SYN.kmc_synth_bins_range.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_double, C.c_uint32, C.c_uint32,
                                              C.c_uint32, C.c_int, C.POINTER(C.POINTER(u8p)), C.POINTER(u64p), C.POINTER(u64p),
                                              C.POINTER(C.POINTER(u64p)), C.POINTER(u64p), C.POINTER(u64p)]
        _SYN.kmc_synth_free.argtypes = [C.c_void_p]
        _SYN.kmc_synth_free.restype = None
        _SYN.kmc_synth_chunk_reads.restype = C.c_uint64
        _SYN.kmc_synth_fastq.restype = C.c_uint64
        _SYN.kmc_synth_fastq.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_double, C.c_char_p, C.c_int]
    return _SYN


def synth_chunk_reads() -> int:
    """read ranges given to synth_bins(read_begin=...) must start on a multiple of this"""
    return int(_syn().kmc_synth_chunk_reads())


class SynthBins:
    """Bin images made by libkmc_synth.so, as zero-copy views into its buffers (valid until close())."""

    def __init__(self, handle, bins):
        self._h = handle
        self.bins = bins  # list of (image uint8 view, n_rec, pack_bytes uint64 view, n_super)

    def close(self):
        if self._h:
            self.bins = []
            _syn().kmc_synth_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def synth_bins(seed: int, genome_len: int, n_reads: int, k: int, n_bins: int = 1, read_len: int = 150, err: float = 0.01,
               sig_len: int = 9, n_threads: int = 0, read_begin: int = 0, read_end=None, copy: bool = True):
    """Bins of reads [read_begin, read_end) (default: all n_reads) of the model. copy=True returns a list of
    (image uint8 ndarray, n_rec, pack_bytes uint64 ndarray, n_super) per bin; copy=False returns a SynthBins holding views."""
    S = _syn()
    if read_end is None:
        read_end = n_reads
    imgs, sizes, nrec, packs, npacks, nsup = C.POINTER(u8p)(), u64p(), u64p(), C.POINTER(u64p)(), u64p(), u64p()
    h = S.kmc_synth_bins_range(seed, genome_len, read_begin, read_end, read_len, err, k, sig_len, n_bins, n_threads, C.byref(imgs),
                               C.byref(sizes), C.byref(nrec), C.byref(packs), C.byref(npacks), C.byref(nsup))
    if not h:
        raise ValueError("kmc_synth_bins: bad arguments or out of memory")
    out = []
    for b in range(n_bins):
        sz = sizes[b]
        img = np.ctypeslib.as_array(imgs[b], shape=(sz,)) if sz else np.zeros(0, dtype=np.uint8)
        pk = np.ctypeslib.as_array(packs[b], shape=(npacks[b],)) if npacks[b] else np.zeros(0, dtype=np.uint64)
        if copy:
            img, pk = img.copy(), pk.copy()
        out.append((img, int(nrec[b]), pk, int(nsup[b])))
    if copy:
        S.kmc_synth_free(h)
        return out
    return SynthBins(h, out)


def synth_fastq(path: str, seed: int, genome_len: int, n_reads: int, read_len: int = 150, err: float = 0.01, n_threads: int = 0,
                read_begin: int = 0) -> int:
    """The same reads synth_bins() cuts into bins, as FASTQ (for the reference kmc). Returns bytes written."""
    n = _syn().kmc_synth_fastq(seed, genome_len, read_begin, n_reads, read_len, err, path.encode(), n_threads)
    if not n:
        raise OSError(f"kmc_synth_fastq could not write {path}")
    return int(n)
