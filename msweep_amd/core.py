"""ctypes binding of libmsweep_core.so (the C ABI in include/msweep_core.h).

Fails loudly when the HIP extension is missing or no GPU is visible: there is no CPU
fallback in the product path (the CPU oracle under oracle/ is test infrastructure and is
never imported from here).
"""
import ctypes as C
import os

import numpy as np

from .buildlib import source_hash  # (sha256 prefix over the library's sources: one definition, buildlib.py)

_HERE = os.path.dirname(os.path.abspath(__file__))
# MSWEEP_CORE_LIB: developer override for A/B timing of two builds in one job
LIB_PATH = os.environ.get("MSWEEP_CORE_LIB") or os.path.join(_HERE, "libmsweep_core.so")

ALGO_RCG, ALGO_EM = 0, 1
PREC_DOUBLE, PREC_FLOAT = 0, 1
TEXT_PROBS, TEXT_LOGL, TEXT_BITSEQ = 0, 1, 2      # msw_core_text_block
ASSIGN_UNASSIGNED, ASSIGN_KEEP_TABLE = 1, 2       # msw_core_assign_reads flags
# msw_core_set_option ids (include/msweep_core.h): the knobs of rcgpar's loops that are restated from memory
OPT_CHECK_EVERY, OPT_INIT_BOUND, OPT_EM_PRIOR, OPT_EM_STOP = 0, 1, 2, 3
_OPTS = {"check_every": OPT_CHECK_EVERY, "init_bound": OPT_INIT_BOUND, "em_prior": OPT_EM_PRIOR, "em_stop": OPT_EM_STOP}

# every symbol include/msweep_core.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "msw_core_create", "msw_core_destroy", "msw_last_error", "msw_core_version",
    "msw_core_set_dense_logl", "msw_core_set_csr", "msw_core_build_likelihood",
    "msw_core_get_dense_logl", "msw_core_layout_hash", "msw_core_shape", "msw_alignment_read",
    "msw_alignment_shape", "msw_alignment_export", "msw_alignment_view", "msw_alignment_destroy", "msw_alignment_last_error",
    "msw_alignment_read_device", "msw_core_build_likelihood_aln", "msw_core_trim", "msw_alignment_on_device", "msw_core_solve", "msw_core_prepare", "msw_core_run",
    "msw_core_gamma",
    "msw_core_trace", "msw_core_set_trace_theta", "msw_core_bootstrap",
    "msw_core_resample_counts", "msw_core_set_profiling", "msw_core_last_timing",
    "msw_core_set_fixed_iters", "msw_core_hbm_stream_rates", "msw_comm_unique_id", "msw_comm_create_rccl", "msw_comm_create_local",
    "msw_comm_destroy", "msw_core_set_comm", "msw_comm_last_error", "msw_core_bootstrap_dist",
    "msw_comm_size", "msw_comm_rccl_count", "msw_comm_allgather", "msw_comm_allreduce", "msw_comm_create_shm", "msw_core_continue", "msw_core_gamma_block",
    "msw_core_last_bootstrap_timing", "msw_core_layout_info", "msw_core_guarded_visits", "msw_core_set_pack_schedule",
    "msw_core_set_option", "msw_core_get_option", "msw_core_bin_reads", "msw_core_bin_reads_aln",
    "msw_core_assign_reads", "msw_core_assign_reads_aln", "msw_core_assign_table_rows", "msw_core_assign_table_block",
    "msw_core_assign_table_block_gzip",
    "msw_core_sparse_probs_begin", "msw_core_sparse_probs_next", "msw_core_sparse_probs_next_gzip",
    "msw_core_last_sparse_probs_timing",
    "msw_core_text_block", "msw_core_format_g6", "msw_core_last_text_timing",
    "msw_core_gzip_begin", "msw_core_text_block_gzip", "msw_core_gzip_append", "msw_core_gzip_end", "msw_core_last_gzip_timing",
    "msw_core_inflate_gzip", "msw_alignment_last_inflate", "msw_alignment_subset",
    "msw_core_set_dense_logl_file", "msw_core_set_dense_logl_text", "msw_core_likfile_counts",
    "msw_fastq_open", "msw_fastq_select", "msw_fastq_next", "msw_fastq_next_gzip", "msw_fastq_last_timing", "msw_fastq_close",
]

# msw_inflate_info.fallback_reason
INFLATE_REASONS = ("none", "forced", "header", "probe mismatch", "chunk status", "crc", "trailing bytes", "memory", "long span")


class MswError(RuntimeError):
    """Non-zero return from the C ABI (mirrors the std::runtime_error the C++ shim throws)."""


class InflateInfo(C.Structure):
    """msw_inflate_info: how a gzip input was inflated (Core.inflate_gzip, Core.last_inflate)"""
    _fields_ = [("payload_bytes", C.c_uint64), ("text_bytes", C.c_uint64), ("chunk_bytes", C.c_uint32), ("n_chunks", C.c_uint32),
                ("n_starts", C.c_uint32), ("on_device", C.c_int32), ("fallback_reason", C.c_int32), ("n_members", C.c_uint32),
                ("kernel_ms", C.c_double),
                ("upload_ms", C.c_double), ("probe_ms", C.c_double), ("window_ms", C.c_double), ("chain_ms", C.c_double),
                ("write_ms", C.c_double), ("crc_ms", C.c_double)]

    def as_dict(self):
        d = {name: getattr(self, name) for name, _ in self._fields_}
        d["reason"] = INFLATE_REASONS[self.fallback_reason] if 0 <= self.fallback_reason < len(INFLATE_REASONS) else "?"
        return d


# msw_likfile_info.reason (include/msweep_core.h: MSW_LIKFILE_*)
LIKFILE_REASONS = ("none", "forced", "open / read", "bad byte", "bad token", "column count", "empty", "too many host cells",
                   "range error", "memory", "too many lines")


class LikFileInfo(C.Structure):
    """msw_likfile_info: whether the device served a --read-likelihood file (Core.set_dense_logl_file), and how"""
    _fields_ = [("text_bytes", C.c_uint64), ("n_ecs", C.c_uint64), ("n_host_cells", C.c_uint64), ("served", C.c_int32),
                ("reason", C.c_int32), ("upload_ms", C.c_double), ("kernel_ms", C.c_double), ("inflate", InflateInfo)]

    def as_dict(self):
        d = {name: getattr(self, name) for name, _ in self._fields_ if name != "inflate"}
        d["inflate"] = self.inflate.as_dict()
        d["reason_text"] = LIKFILE_REASONS[self.reason] if 0 <= self.reason < len(LIKFILE_REASONS) else "?"
        return d


# msw_fastq_info.reason
FASTQ_REASONS = ("none", "line count", "no '@'", "no '+'", "lengths differ")


class FastqInfo(C.Structure):
    """msw_fastq_info: what Core.fastq_open found -- records, bytes of text, how the file was inflated, the stage times"""
    _fields_ = [("n_records", C.c_uint64), ("text_bytes", C.c_uint64), ("reason", C.c_int32), ("bad_record", C.c_uint64),
                ("inflate", InflateInfo), ("index_ms", C.c_double), ("upload_ms", C.c_double)]

    def as_dict(self):
        d = {name: getattr(self, name) for name, _ in self._fields_ if name != "inflate"}
        d["inflate"] = self.inflate.as_dict()
        d["reason_text"] = FASTQ_REASONS[self.reason] if 0 <= self.reason < len(FASTQ_REASONS) else "?"
        return d


class Timing(C.Structure):
    _fields_ = [("solve_ms", C.c_double), ("passA_ms", C.c_double), ("passB_ms", C.c_double),
                ("passA_launches", C.c_uint64), ("passB_launches", C.c_uint64), ("iters", C.c_uint64),
                ("bytes_passA", C.c_uint64), ("bytes_passB", C.c_uint64), ("collective_ms", C.c_double),
                ("collectives", C.c_uint64), ("em_float_kernels", C.c_uint64)]


class LayoutInfo(C.Structure):
    _fields_ = [("record_bytes", C.c_int32), ("index_records", C.c_int32), ("groups_in_lds", C.c_int32),
                ("table_in_lds", C.c_int32), ("passB_mode", C.c_int32), ("slot_entries", C.c_uint32),
                ("slot_entries_in_lds", C.c_uint32), ("n_slices", C.c_uint32), ("n_long_ecs", C.c_uint32),
                ("rows", C.c_uint64), ("rows_from_memory", C.c_uint64), ("slices_by_lanes", C.c_uint32 * 7),
                ("max_rows", C.c_uint32), ("bank_scheduled", C.c_int32), ("passB_reg_cells", C.c_int32),
                ("rows_over_8", C.c_uint64), ("passB_waves", C.c_int32), ("pad_", C.c_int32)]


class BootstrapTiming(C.Structure):
    _fields_ = [("table_ms", C.c_double), ("solve_ms", C.c_double), ("gather_ms", C.c_double),
                ("replicates", C.c_uint64), ("iterations", C.c_uint64), ("table_reused", C.c_uint64)]


_lib = None


def _check_fresh(L):
    """A library that was not compiled from the sources in this tree is refused (MSWEEP_CORE_LIB, the
    developer override for A/B builds, is exempt): a stale prebuilt .so cannot pass silently."""
    if os.environ.get("MSWEEP_CORE_LIB"):
        return
    ver = L.msw_core_version().decode()
    try:
        want = source_hash()
    except OSError:
        return          # installed without its sources: nothing to compare with
    if not ver.endswith("src " + want):
        raise MswError(f"{LIB_PATH} is stale: built from other sources ({ver}; the tree hashes to {want}). "
                       "Rebuild: python -c 'import __graft_entry__ as g; g.build()'")


def load_library():
    """dlopen the in-tree extension; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MswError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    vp, sz, dp = C.c_void_p, C.c_size_t, C.c_double
    L.msw_core_version.restype = C.c_char_p
    _check_fresh(L)
    L.msw_core_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.msw_core_destroy.argtypes = [vp]
    L.msw_core_destroy.restype = None
    L.msw_last_error.argtypes = [vp]
    L.msw_last_error.restype = C.c_char_p
    L.msw_core_version.restype = C.c_char_p
    L.msw_core_set_dense_logl.argtypes = [vp, vp, sz, sz, sz]
    L.msw_core_set_csr.argtypes = [vp, vp, vp, vp, vp, sz, dp, sz, sz]
    L.msw_core_set_dense_logl_file.argtypes = [vp, C.c_char_p, sz, C.POINTER(LikFileInfo)]
    L.msw_core_set_dense_logl_text.argtypes = [vp, vp, sz, sz, C.POINTER(LikFileInfo)]
    L.msw_core_likfile_counts.argtypes = [vp, vp, sz]
    L.msw_core_build_likelihood.argtypes = [vp, vp, vp, sz, vp, sz, vp, sz, vp, dp, dp, dp, sz,
                                            C.POINTER(sz), vp, vp]
    L.msw_core_get_dense_logl.argtypes = [vp, vp, sz]
    L.msw_core_layout_hash.argtypes = [vp, vp]
    L.msw_core_shape.argtypes = [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    L.msw_core_solve.argtypes = [vp, vp, vp, dp, sz, C.c_int, C.c_int, vp, C.POINTER(sz), C.POINTER(dp)]
    L.msw_core_prepare.argtypes = [vp, vp, vp]
    L.msw_core_run.argtypes = [vp, dp, sz, C.c_int, C.c_int, vp, C.POINTER(sz), C.POINTER(dp)]
    L.msw_core_continue.argtypes = [vp, sz, vp, C.POINTER(sz), C.POINTER(dp)]
    L.msw_core_gamma.argtypes = [vp, vp, sz]
    L.msw_core_gamma_block.argtypes = [vp, sz, sz, vp, sz]
    L.msw_core_bin_reads.argtypes = [vp, vp, vp, sz, vp, vp, sz, vp, vp, vp]
    L.msw_core_bin_reads_aln.argtypes = [vp, vp, vp, vp, sz, vp, vp, vp]
    if hasattr(L, "msw_core_assign_reads"):     # (a library of an earlier commit behind MSWEEP_CORE_LIB has none of them)
        L.msw_core_assign_reads.argtypes = [vp, vp, vp, sz, vp, vp, sz, C.c_uint, vp, vp, vp, vp]
        L.msw_core_assign_reads_aln.argtypes = [vp, vp, vp, vp, sz, C.c_uint, vp, vp, vp, vp]
        L.msw_core_assign_table_rows.argtypes = [vp, C.POINTER(sz)]
        L.msw_core_assign_table_block.argtypes = [vp, sz, sz, C.POINTER(vp), C.POINTER(sz)]
        L.msw_core_assign_table_block_gzip.argtypes = [vp, sz, sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz)]
    L.msw_core_text_block.argtypes = [vp, C.c_int, sz, sz, vp, sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz)]
    L.msw_core_format_g6.argtypes = [vp, vp, sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz)]
    L.msw_core_last_text_timing.argtypes = [vp, C.POINTER(dp), C.POINTER(C.c_uint64)]
    L.msw_core_gzip_begin.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(sz)]
    L.msw_core_text_block_gzip.argtypes = [vp, C.c_int, sz, sz, vp, sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    L.msw_core_gzip_append.argtypes = [vp, vp, sz, C.POINTER(vp), C.POINTER(sz)]
    L.msw_core_gzip_end.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
    L.msw_core_last_gzip_timing.argtypes = [vp, C.POINTER(dp), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.msw_core_inflate_gzip.argtypes = [vp, vp, sz, sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(InflateInfo)]
    L.msw_alignment_last_inflate.argtypes = [vp, C.POINTER(InflateInfo), sz, C.POINTER(sz)]
    L.msw_core_sparse_probs_begin.argtypes = [vp, vp, C.c_double, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    L.msw_core_sparse_probs_next.argtypes = [vp, sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                             C.POINTER(sz)]
    L.msw_core_sparse_probs_next_gzip.argtypes = [vp, sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_uint64), C.POINTER(sz)]
    L.msw_core_last_sparse_probs_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.msw_fastq_open.argtypes = [vp, C.c_char_p, C.POINTER(vp), C.POINTER(FastqInfo)]
    L.msw_fastq_select.argtypes = [vp, vp, vp, sz, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.msw_fastq_next.argtypes = [vp, vp, sz, C.POINTER(vp), C.POINTER(sz)]
    L.msw_fastq_next_gzip.argtypes = [vp, vp, sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz)]
    L.msw_fastq_last_timing.argtypes = [vp, C.POINTER(dp), C.POINTER(C.c_uint64)]
    L.msw_fastq_close.argtypes = [vp]
    L.msw_fastq_close.restype = None
    L.msw_core_trace.argtypes = [vp, sz, vp, vp, vp, vp, vp, C.POINTER(sz)]
    L.msw_core_set_trace_theta.argtypes = [vp, sz]
    L.msw_core_bootstrap.argtypes = [vp, vp, C.c_int32, sz, sz, sz, vp, dp, sz, C.c_int, C.c_int, vp, vp]
    L.msw_core_resample_counts.argtypes = [vp, vp, sz, C.c_int32, sz, sz, sz, vp]
    L.msw_core_bootstrap_dist.argtypes = [vp, vp, vp, C.c_int32, sz, sz, vp, dp, sz, C.c_int, C.c_int, vp, vp]
    L.msw_comm_size.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.msw_comm_rccl_count.argtypes = [vp, C.POINTER(C.c_int)]
    L.msw_comm_allgather.argtypes = [vp, vp, sz, vp]
    L.msw_comm_allreduce.argtypes = [vp, vp, sz, vp, sz, C.c_int, C.POINTER(dp)]
    L.msw_comm_create_shm.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.msw_core_set_profiling.argtypes = [vp, C.c_int]
    L.msw_core_set_fixed_iters.argtypes = [vp, C.c_int]
    L.msw_core_set_pack_schedule.argtypes = [vp, C.c_int]
    L.msw_core_set_option.argtypes = [vp, C.c_int, C.c_double]
    L.msw_core_get_option.argtypes = [vp, C.c_int, C.POINTER(C.c_double)]
    L.msw_core_hbm_stream_rates.argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.msw_core_last_timing.argtypes = [vp, C.POINTER(Timing)]
    L.msw_core_last_bootstrap_timing.argtypes = [vp, C.POINTER(BootstrapTiming)]
    L.msw_core_guarded_visits.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.msw_core_layout_info.argtypes = [vp, C.POINTER(LayoutInfo)]
    L.msw_comm_unique_id.argtypes = [vp]
    L.msw_comm_create_rccl.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.msw_comm_create_local.argtypes = [C.c_int, C.POINTER(vp)]
    L.msw_comm_destroy.argtypes = [vp]
    L.msw_comm_destroy.restype = None
    L.msw_core_set_comm.argtypes = [vp, vp]
    L.msw_comm_last_error.restype = C.c_char_p
    L.msw_alignment_read.argtypes = [C.POINTER(C.c_char_p), sz, sz, C.c_int, C.POINTER(vp)]
    L.msw_alignment_shape.argtypes = [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    L.msw_alignment_view.argtypes = [vp] + [C.POINTER(vp)] * 5
    L.msw_alignment_export.argtypes = [vp, vp, vp, vp, vp, vp]
    L.msw_alignment_destroy.argtypes = [vp]
    L.msw_core_trim.argtypes = [vp]
    L.msw_alignment_on_device.argtypes = [vp]
    L.msw_alignment_read_device.argtypes = [vp, C.POINTER(C.c_char_p), sz, sz, C.c_int, C.POINTER(vp)]
    L.msw_core_build_likelihood_aln.argtypes = [vp, vp, vp, sz, vp, sz, C.c_double, C.c_double, C.c_double, sz,
                                                C.POINTER(sz), vp, vp]
    L.msw_alignment_subset.argtypes = [vp, vp, vp, sz, vp, C.POINTER(vp), C.POINTER(sz)]
    L.msw_alignment_destroy.restype = None
    L.msw_alignment_last_error.restype = C.c_char_p
    _lib = L
    return L


class _AlignmentOwner:
    """Keeps a native alignment handle alive for as long as an array that views its storage is."""

    def __init__(self, L, h):
        self._L, self._h = L, h

    def __del__(self):
        try:
            if self._h:
                self._L.msw_alignment_destroy(self._h)
                self._h = None
        except Exception:
            pass


def read_alignment(paths, n_targets, merge_mode="intersection", copy=False):
    """Native Themisto plaintext reader + EC collapse (msw_alignment_*, host code of the library):
    dict(ec_tptr, ec_targets, ec_counts, ec_rptr, ec_reads, n_reads).  Errors carry the reference's
    messages (include/mSWEEP_alignment.hpp:84-91, :131).  The arrays are read-only VIEWS of the native handle's own
    storage (msw_alignment_view: no 0.9 GB copy at cfg3), which lives as long as any of them does; copy=True gives
    ordinary writable arrays (msw_alignment_export)."""
    L = load_library()
    if merge_mode not in ("intersection", "union"):
        raise MswError(f"Unrecognized option `{merge_mode}` for --themisto-mode")
    arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
    h = C.c_void_p()
    if L.msw_alignment_read(arr, len(paths), int(n_targets), 0 if merge_mode == "intersection" else 1, C.byref(h)):
        raise MswError(L.msw_alignment_last_error().decode())
    owner = _AlignmentOwner(L, h)
    ne, nr, nh, na = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    L.msw_alignment_shape(h, C.byref(ne), C.byref(nr), C.byref(nh), C.byref(na))
    if copy:
        out = dict(ec_tptr=np.empty(ne.value + 1, np.uint64), ec_targets=np.empty(nh.value, np.uint32),
                   ec_counts=np.empty(ne.value, np.uint64), ec_rptr=np.empty(ne.value + 1, np.uint64),
                   ec_reads=np.empty(na.value, np.uint32), n_reads=int(nr.value))
        if L.msw_alignment_export(h, _ptr(out["ec_tptr"]), _ptr(out["ec_targets"]), _ptr(out["ec_counts"]),
                                  _ptr(out["ec_rptr"]), _ptr(out["ec_reads"])):
            raise MswError("msw_alignment_export failed")
        return out
    return _alignment_views(L, h, owner, ne.value, nh.value, na.value, nr.value)


def read_alignment_handle(paths, n_targets, merge_mode="intersection"):
    """read_alignment() as a handle (a DeviceAlignment whose arrays are host-resident: on_device is False): what
    subset_alignment() takes and returns.  No GPU is touched."""
    L = load_library()
    if merge_mode not in ("intersection", "union"):
        raise MswError(f"Unrecognized option `{merge_mode}` for --themisto-mode")
    arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
    h = C.c_void_p()
    if L.msw_alignment_read(arr, len(paths), int(n_targets), 0 if merge_mode == "intersection" else 1, C.byref(h)):
        raise MswError(L.msw_alignment_last_error().decode())
    a = DeviceAlignment(L, h)
    a.n_targets = int(n_targets)
    return a


def _subset(L, core_h, aln, read_ids, keep):
    read_ids = _arr(read_ids, np.uint32)
    keep = _arr(np.asarray(keep) != 0, np.uint8)
    n_targets = getattr(aln, "n_targets", None)
    if n_targets is not None and len(keep) != n_targets:
        raise MswError(f"subset_alignment: keep has {len(keep)} entries, the alignment {n_targets} target sequences")
    h, nt = C.c_void_p(), C.c_size_t()
    if L.msw_alignment_subset(core_h, aln._h, _ptr(read_ids) if len(read_ids) else None, len(read_ids), _ptr(keep),
                              C.byref(h), C.byref(nt)):
        raise MswError(L.msw_last_error(core_h).decode())
    out = DeviceAlignment(L, h)
    out.n_targets = int(nt.value)
    return out


def subset_alignment(aln, read_ids, keep):
    """msw_alignment_subset without a handle, for a HOST-resident alignment (read_alignment_handle, or a Core.read_alignment
    the host parser served): the alignment restricted to the reads `read_ids` and the target sequences with keep[t] != 0,
    collapsed into classes again -- kept targets renumbered by rank, read ids as they are (include/msweep_core.h states
    the contract).  Returns a handle like `aln` with .n_targets = the number of kept sequences.  No GPU is touched."""
    return _subset(load_library(), None, aln, read_ids, keep)


class DeviceAlignment:
    """An alignment read by msw_alignment_read_device: its arrays live in the memory of the GPU that parsed the text
    (Core.read_alignment).  Core.build_likelihood_aln consumes them there; arrays() copies them out on first use
    (the dict read_alignment returns, as read-only views)."""

    def __init__(self, L, h):
        self._L, self._h = L, h
        self._owner = _AlignmentOwner(L, h)
        ne, nr, nh, na = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        L.msw_alignment_shape(h, C.byref(ne), C.byref(nr), C.byref(nh), C.byref(na))
        self.n_ecs, self.n_reads, self.n_hits, self.n_aligned = ne.value, nr.value, nh.value, na.value
        self._arrays = None
        self._counts = None
        self.on_device = bool(L.msw_alignment_on_device(h))   # False: the host parser took the text (its word is final)

    def ec_counts(self):
        """reads per class (uint64): the one array the drivers need on the host -- 8 bytes per class leave the device"""
        if self._counts is None:
            out = np.empty(self.n_ecs, np.uint64)
            if self._L.msw_alignment_export(self._h, None, None, _ptr(out), None, None):
                raise MswError("msw_alignment_export failed")
            self._counts = out
        return self._counts

    def close(self):
        """Gives the alignment's memory back now, not when the last reference goes (a driver that reads one sample after
        the other on one handle).  Arrays handed out by arrays() keep it alive as before."""
        if self._arrays is None and self._owner._h:
            self._L.msw_alignment_destroy(self._owner._h)
            self._owner._h = None
        self._h = None

    def arrays(self):
        if self._arrays is None:
            self._arrays = _alignment_views(self._L, self._h, self._owner, self.n_ecs, self.n_hits, self.n_aligned, self.n_reads)
        return self._arrays


def _alignment_views(L, h, owner, n_ecs, n_hits, n_aligned, n_reads):
    p = [C.c_void_p() for _ in range(5)]
    if L.msw_alignment_view(h, *[C.byref(x) for x in p]):
        raise MswError("msw_alignment_view failed")

    def view(ptr, n, ctype, dtype):
        if n == 0 or not ptr.value:
            return np.empty(0, dtype)
        buf = (ctype * n).from_address(ptr.value)
        buf._owner = owner               # array -> ctypes buffer -> owner -> handle
        a = np.frombuffer(buf, dtype=dtype)
        a.flags.writeable = False
        return a
    return dict(ec_tptr=view(p[0], n_ecs + 1, C.c_uint64, np.uint64), ec_targets=view(p[1], n_hits, C.c_uint32, np.uint32),
                ec_counts=view(p[2], n_ecs, C.c_uint64, np.uint64), ec_rptr=view(p[3], n_ecs + 1, C.c_uint64, np.uint64),
                ec_reads=view(p[4], n_aligned, C.c_uint32, np.uint32), n_reads=int(n_reads))


class Fastq:
    """A read file resident on a Core's device with the index of its records (msw_fastq_open): select read ids, then take
    their records in pieces -- plain bytes, or bytes of the handle's open gzip stream.  Closed by close(), or with its
    Core."""

    def __init__(self, core, h, info):
        self._core, self._h, self.info = core, h, info

    def _handle(self):
        if not self._h or not self._core._h:
            raise MswError("the read file is closed")
        return self._h

    def select(self, ids):
        """Replaces the selection by the records `ids` names (0-based, any order, repeats allowed): ascending, each once.
        Returns (distinct records, their bytes)."""
        ids = _arr(ids, np.uint32)
        if ids.ndim != 1:
            raise MswError("Fastq.select: ids must be a 1-D array")
        n, nb = C.c_uint64(), C.c_uint64()
        c = self._core
        c._check(c._L.msw_fastq_select(c._h, self._handle(), _ptr(ids) if len(ids) else None, len(ids), C.byref(n), C.byref(nb)))
        return n.value, nb.value

    def pieces(self, max_bytes=256 << 20):
        """The selection's records in file order, whole records in pieces of at most max_bytes (msw_fastq_next)."""
        c = self._core
        while True:
            p, n = C.c_void_p(), C.c_size_t()
            c._check(c._L.msw_fastq_next(c._h, self._handle(), int(max_bytes), C.byref(p), C.byref(n)))
            if not n.value:
                return
            yield C.string_at(p.value, n.value)

    def pieces_gzip(self, max_bytes=256 << 20):
        """The same inside the Core's open gzip stream (msw_fastq_next_gzip): per piece the bytes to append to the file
        (zlib on the host, MSWEEP_HOST_GZIP=1, may hold a piece's bytes back: b"")."""
        c = self._core
        while True:
            p, n, nt = C.c_void_p(), C.c_size_t(), C.c_size_t()
            c._check(c._L.msw_fastq_next_gzip(c._h, self._handle(), int(max_bytes), C.byref(p), C.byref(n), C.byref(nt)))
            if not nt.value:
                return
            yield C.string_at(p.value, n.value) if n.value else b""

    def close(self):
        if self._h and self._core._h:
            self._core._L.msw_fastq_close(self._h)
        self._h = None
        if self in self._core._fastqs:
            self._core._fastqs.remove(self)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class SparseProbs:
    """The selection msw_core_sparse_probs_begin left on a Core: the cells with probability >= threshold as lines
    "id\tg\tp\n", rows by EC or by aligned read.  .rows, .log_threshold; the text in pieces of whole rows -- plain bytes, or
    bytes of the Core's open gzip stream.  A new likelihood, a solve, a bootstrap or Core.trim() ends it."""

    def __init__(self, core, rows, log_threshold):
        self._core, self.rows, self.log_threshold = core, rows, log_threshold
        self.cells = self.host_cells = 0    # kept cells / cells the host printed, over the pieces taken so far

    def pieces(self, max_bytes=256 << 20):
        """The text of the next whole rows, at most max_bytes per piece (msw_core_sparse_probs_next)."""
        c = self._core
        while True:
            p, n, done, nc, nh = C.c_void_p(), C.c_size_t(), C.c_uint64(), C.c_uint64(), C.c_size_t()
            c._check(c._L.msw_core_sparse_probs_next(c._h, int(max_bytes), C.byref(p), C.byref(n), C.byref(done), C.byref(nc),
                                                     C.byref(nh)))
            self.cells += nc.value
            self.host_cells += nh.value
            if n.value:
                yield C.string_at(p.value, n.value)
            if done.value >= self.rows:
                return

    def pieces_gzip(self, max_bytes=256 << 20):
        """The same inside the Core's open gzip stream (msw_core_sparse_probs_next_gzip): per piece the bytes to append to
        the file (zlib on the host, MSWEEP_HOST_GZIP=1, may hold a piece's bytes back: b"")."""
        c = self._core
        while True:
            p, n, done, nt = C.c_void_p(), C.c_size_t(), C.c_uint64(), C.c_size_t()
            c._check(c._L.msw_core_sparse_probs_next_gzip(c._h, int(max_bytes), C.byref(p), C.byref(n), C.byref(done), C.byref(nt)))
            if nt.value:
                yield C.string_at(p.value, n.value) if n.value else b""
            if done.value >= self.rows:
                return

    def last_timing(self):
        """(ms of the kernels since begin -- device events --, text bytes they wrote, kept cells)"""
        c = self._core
        ms, nb, nc = C.c_double(), C.c_uint64(), C.c_uint64()
        c._check(c._L.msw_core_last_sparse_probs_timing(c._h, C.byref(ms), C.byref(nb), C.byref(nc)))
        return ms.value, nb.value, nc.value


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _arr(x, dt):
    return np.ascontiguousarray(x, dtype=dt)


class Core:
    """One handle = one GPU + one resident likelihood (the object rcg_optl() would receive)."""

    def __init__(self, device=0):
        self._L = load_library()
        self._h = C.c_void_p()
        rc = self._L.msw_core_create(int(device), C.byref(self._h))
        if rc != 0:
            raise MswError(self._L.msw_last_error(None).decode())
        self.device = device
        self.generation = 0     # solves started on this handle (rcgpar.EcProbs: whose state gamma() would read)
        self._fastqs = []       # read files open on this handle (fastq_open): closed with it

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            for fq in list(getattr(self, "_fastqs", [])):
                fq.close()
            self._L.msw_core_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise MswError(self._L.msw_last_error(self._h).decode())

    # ---- likelihood -------------------------------------------------------------------
    def set_dense_logl(self, logl):
        """logl: G x E array, rows = groups (seamat layout of Likelihood::log_mat())."""
        logl = np.asarray(logl, dtype=np.float64)
        if logl.ndim != 2:
            raise MswError("set_dense_logl: expected a 2-D G x E array")
        if logl.strides[1] != 8 or logl.strides[0] % 8 or logl.strides[0] < 8 * logl.shape[1]:
            logl = np.ascontiguousarray(logl)
        G, E = logl.shape
        # (a single row's stride is arbitrary in numpy: its leading dimension is the row itself)
        self._check(self._L.msw_core_set_dense_logl(self._h, _ptr(logl), G, E, logl.strides[0] // 8 if G > 1 else E))

    def _likfile_result(self, info):
        d = info.as_dict()
        counts = None
        if d["served"]:
            counts = np.empty(d["n_ecs"], np.uint64)
            self._check(self._L.msw_core_likfile_counts(self._h, _ptr(counts), len(counts)))
        return d, counts

    def set_dense_logl_file(self, path, n_groups):
        """--read-likelihood on the device (msw_core_set_dense_logl_file): (info, counts).  info["served"] = 1: the file --
        plain, gzip or BGZF -- was parsed by the kernels, the handle holds what set_dense_logl would leave from its matrix and
        counts is its first column (uint64).  served = 0: nothing changed on the handle, counts is None and info["reason_text"]
        says why; the caller parses the file itself."""
        info = LikFileInfo()
        self._check(self._L.msw_core_set_dense_logl_file(self._h, os.fsencode(path), int(n_groups), C.byref(info)))
        return self._likfile_result(info)

    def set_dense_logl_text(self, text, n_groups):
        """set_dense_logl_file on plain text in host memory (bytes): the parser's test and diagnostic entry"""
        text = bytes(text)
        info = LikFileInfo()
        self._check(self._L.msw_core_set_dense_logl_text(self._h, text if text else None, len(text), int(n_groups), C.byref(info)))
        return self._likfile_result(info)

    def set_csr(self, rowptr, grp, cnt, lut, logzi, n_groups):
        rowptr = _arr(rowptr, np.uint64)
        grp = _arr(grp, np.uint32)
        cnt = _arr(cnt, np.uint32)
        lut = _arr(lut, np.float64)
        if lut.ndim != 2 or lut.shape[0] != n_groups:
            raise MswError("set_csr: lut must be n_groups x lut_ld")
        if len(grp) != len(cnt) or (len(rowptr) and int(rowptr[-1]) != len(grp)):
            raise MswError("set_csr: rowptr / grp / cnt lengths disagree")
        E = len(rowptr) - 1
        self._check(self._L.msw_core_set_csr(self._h, _ptr(rowptr), _ptr(grp), _ptr(cnt), _ptr(lut),
                                             lut.shape[1], float(logzi), int(n_groups), E))

    def build_likelihood(self, ec_tptr, ec_targets, target_group, group_sizes, ec_counts, q=0.65, e=0.01,
                         zero_inflation=0.01, min_hits=0, want_logc=True):
        """Device build from the pseudoalignment (replaces LL_WOR21::fill_ll_mat).
        Returns (n_groups_kept, mask[G] bool, logc[E] or None when want_logc is False)."""
        ec_tptr = _arr(ec_tptr, np.uint64)
        ec_targets = _arr(ec_targets, np.uint32)
        target_group = _arr(target_group, np.uint32)
        group_sizes = _arr(group_sizes, np.uint64)
        ec_counts = _arr(ec_counts, np.uint64)
        E, G = len(ec_tptr) - 1, len(group_sizes)
        if len(ec_counts) != E:
            raise MswError("build_likelihood: ec_counts length != n_ecs")
        n_out = C.c_size_t()
        mask = np.zeros(G, np.uint8)
        logc = np.empty(E, np.float64) if want_logc else None
        self._check(self._L.msw_core_build_likelihood(
            self._h, _ptr(ec_tptr), _ptr(ec_targets), E, _ptr(target_group), len(target_group),
            _ptr(group_sizes), G, _ptr(ec_counts), q, e, zero_inflation, int(min_hits), C.byref(n_out),
            _ptr(mask), _ptr(logc)))
        return n_out.value, mask.astype(bool), logc

    def read_alignment(self, paths, n_targets, merge_mode="intersection"):
        """The Themisto plaintext reader ON THIS GPU (msw_alignment_read_device): the text goes to device memory as it
        is read; parse, rows by read id, paired-end merge, the reference's hash, sort and classes are kernels.  Returns
        a DeviceAlignment (build_likelihood_aln reads it where it lies; .arrays() = what read_alignment() returns).
        Errors carry the reference's messages: text the kernels do not judge goes to the host reader."""
        if merge_mode not in ("intersection", "union"):
            raise MswError(f"Unrecognized option `{merge_mode}` for --themisto-mode")
        arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
        h = C.c_void_p()
        if self._L.msw_alignment_read_device(self._h, arr, len(paths), int(n_targets),
                                             0 if merge_mode == "intersection" else 1, C.byref(h)):
            raise MswError(self._L.msw_alignment_last_error().decode())
        a = DeviceAlignment(self._L, h)
        a.n_targets = int(n_targets)
        return a

    def subset_alignment(self, aln, read_ids, keep):
        """msw_alignment_subset on this GPU: `aln` restricted to the reads `read_ids` and the target sequences with
        keep[t] != 0, collapsed into classes again by kernels; the result stays resident (a DeviceAlignment with
        .n_targets = the number of kept sequences: it can be built from, binned, assigned and subset again).  A
        host-resident `aln` is served by the host loops (the module's subset_alignment)."""
        return _subset(self._L, self._h, aln, read_ids, keep)

    def trim(self):
        """Gives the device temporaries of read_alignment back (kept on the handle between calls: msw_core_trim)."""
        self._check(self._L.msw_core_trim(self._h))

    def build_likelihood_aln(self, aln, target_group, group_sizes, q=0.65, e=0.01, zero_inflation=0.01, min_hits=0,
                             want_logc=True):
        """build_likelihood on a DeviceAlignment: its classes, targets and read counts are read in device memory.
        Returns (n_groups_kept, mask[G] bool, logc[E] or None)."""
        target_group = _arr(target_group, np.uint32)
        group_sizes = _arr(group_sizes, np.uint64)
        G = len(group_sizes)
        n_out = C.c_size_t()
        mask = np.zeros(G, np.uint8)
        logc = np.empty(aln.n_ecs, np.float64) if want_logc else None
        self._check(self._L.msw_core_build_likelihood_aln(
            self._h, aln._h, _ptr(target_group), len(target_group), _ptr(group_sizes), G, q, e, zero_inflation,
            int(min_hits), C.byref(n_out), _ptr(mask), _ptr(logc)))
        return n_out.value, mask.astype(bool), logc

    def shape(self):
        g, e, n = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self._check(self._L.msw_core_shape(self._h, C.byref(g), C.byref(e), C.byref(n)))
        return g.value, e.value, n.value

    def layout_info(self):
        """How the resident CSR-of-ECs likelihood is laid out for the sweeps (msw_core_layout_info)."""
        t = LayoutInfo()
        self._check(self._L.msw_core_layout_info(self._h, C.byref(t)))
        return {k: (list(getattr(t, k)) if k == "slices_by_lanes" else getattr(t, k)) for k, _ in LayoutInfo._fields_
                if k != "pad_"}

    def layout_hash(self):
        out = C.c_uint64(0)
        self._check(self._L.msw_core_layout_hash(self._h, C.byref(out)))
        return int(out.value)

    def get_dense_logl(self):
        G, E, _ = self.shape()
        out = np.empty((G, E))
        self._check(self._L.msw_core_get_dense_logl(self._h, _ptr(out), E))
        return out

    # ---- solve --------------------------------------------------------------------------
    def solve(self, logc, alpha0, tol=1e-6, max_iters=5000, algo=ALGO_RCG, prec=PREC_DOUBLE):
        """logc=None: the log counts build_likelihood() left on the device (no upload per solve)."""
        G, E, _ = self.shape()
        logc = None if logc is None else _arr(logc, np.float64)
        alpha0 = _arr(alpha0, np.float64)
        if (logc is not None and len(logc) != E) or len(alpha0) != G:
            raise MswError(f"solve: expected logc[{E}] and alpha0[{G}], got {len(logc)} and {len(alpha0)}")
        theta = np.empty(G)
        it, b = C.c_size_t(), C.c_double()
        self.generation += 1
        self._check(self._L.msw_core_solve(self._h, _ptr(logc), _ptr(alpha0), float(tol), int(max_iters),
                                           int(algo), int(prec), _ptr(theta), C.byref(it), C.byref(b)))
        return dict(theta=theta, iters=it.value, bound=b.value)

    def prepare(self, logc, alpha0):
        """logc=None: the log counts build_likelihood() left on the device."""
        G, E, _ = self.shape()
        logc = None if logc is None else _arr(logc, np.float64)
        alpha0 = _arr(alpha0, np.float64)
        if (logc is not None and len(logc) != E) or len(alpha0) != G:
            raise MswError(f"prepare: expected logc[{E}] and alpha0[{G}], got "
                           f"{None if logc is None else len(logc)} and {len(alpha0)}")
        self._check(self._L.msw_core_prepare(self._h, _ptr(logc), _ptr(alpha0)))

    def run(self, tol=1e-6, max_iters=5000, algo=ALGO_RCG, prec=PREC_DOUBLE):
        G, _, _ = self.shape()
        theta = np.empty(G)
        it, b = C.c_size_t(), C.c_double()
        self.generation += 1
        self._check(self._L.msw_core_run(self._h, float(tol), int(max_iters), int(algo), int(prec), _ptr(theta),
                                         C.byref(it), C.byref(b)))
        return dict(theta=theta, iters=it.value, bound=b.value)

    def continue_(self, n_iters):
        """n_iters more iterations of the fixed-iteration RCG solve that last ran (msw_core_continue)."""
        G, _, _ = self.shape()
        theta = np.empty(G)
        it, b = C.c_size_t(), C.c_double()
        self.generation += 1
        self._check(self._L.msw_core_continue(self._h, int(n_iters), _ptr(theta), C.byref(it), C.byref(b)))
        return dict(theta=theta, iters=it.value, bound=b.value)

    def gamma(self):
        G, E, _ = self.shape()
        out = np.empty((G, E))
        self._check(self._L.msw_core_gamma(self._h, _ptr(out), E))
        return out

    def gamma_block(self, ec_begin, ec_end):
        """G x (ec_end - ec_begin) block of the log-responsibilities (msw_core_gamma_block)."""
        G, E, _ = self.shape()
        w = int(ec_end) - int(ec_begin)
        out = np.empty((G, max(w, 0)))
        self._check(self._L.msw_core_gamma_block(self._h, int(ec_begin), int(ec_end), _ptr(out), max(w, 1)))
        return out

    def text_block(self, what, ec_begin, ec_end, line_prefix=None, n_zero_cols=0, with_host_cells=False):
        """The lines of the ECs [ec_begin, ec_end) of a matrix output, formatted on the device (msw_core_text_block):
        TEXT_PROBS (--write-probs), TEXT_LOGL (--write-likelihood; line_prefix = the read count of every class) or
        TEXT_BITSEQ (the BitSeq line after the read id).  Returns the bytes -- a copy: the library's buffer lives until
        the next call only -- and, with_host_cells, how many cells the host had to format."""
        if line_prefix is not None:
            line_prefix = _arr(line_prefix, np.uint64)
            if len(line_prefix) != int(ec_end) - int(ec_begin):
                raise MswError("text_block: one line_prefix per class of the range")
        p, n, nh = C.c_void_p(), C.c_size_t(), C.c_size_t()
        self._check(self._L.msw_core_text_block(self._h, int(what), int(ec_begin), int(ec_end), _ptr(line_prefix),
                                                int(n_zero_cols), C.byref(p), C.byref(n), C.byref(nh)))
        text = C.string_at(p.value, n.value) if n.value else b""
        return (text, nh.value) if with_host_cells else text

    def format_g6(self, x, with_host_cells=False):
        """printf("%g") of every double of x on the device, one per line (msw_core_format_g6: the formatter's test and
        diagnostic entry)."""
        x = _arr(x, np.float64).ravel()
        p, n, nh = C.c_void_p(), C.c_size_t(), C.c_size_t()
        self._check(self._L.msw_core_format_g6(self._h, _ptr(x) if len(x) else None, len(x), C.byref(p), C.byref(n), C.byref(nh)))
        text = C.string_at(p.value, n.value) if n.value else b""
        return (text, nh.value) if with_host_cells else text

    def last_text_timing(self):
        """(device ms of the text kernels, bytes they wrote) of the last text_block / format_g6 call"""
        ms, nb = C.c_double(), C.c_uint64()
        self._check(self._L.msw_core_last_text_timing(self._h, C.byref(ms), C.byref(nb)))
        return ms.value, nb.value

    # ---- --compress z: one gzip stream per handle, compressed on the device (msw_core_gzip_*).  Every call returns the
    # bytes to append to the file -- a copy: the library's buffer lives until the next call only.
    def gzip_begin(self, level=6):
        """Opens the stream (level 0 ... 9; 0 stores, 1 ... 9 run the core's one parse); returns the gzip header."""
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._L.msw_core_gzip_begin(self._h, int(level), C.byref(p), C.byref(n)))
        return C.string_at(p.value, n.value) if n.value else b""

    def text_block_gzip(self, what, ec_begin, ec_end, line_prefix=None, n_zero_cols=0, with_info=False):
        """text_block into the open stream (msw_core_text_block_gzip): the compressed chunks of that text and, with_info,
        (cells the host had to format, uncompressed length)."""
        if line_prefix is not None:
            line_prefix = _arr(line_prefix, np.uint64)
            if len(line_prefix) != int(ec_end) - int(ec_begin):
                raise MswError("text_block_gzip: one line_prefix per class of the range")
        p, n, nh, nt = C.c_void_p(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        self._check(self._L.msw_core_text_block_gzip(self._h, int(what), int(ec_begin), int(ec_end), _ptr(line_prefix),
                                                     int(n_zero_cols), C.byref(p), C.byref(n), C.byref(nh), C.byref(nt)))
        out = C.string_at(p.value, n.value) if n.value else b""
        return (out, nh.value, nt.value) if with_info else out

    def gzip_append(self, data):
        """Host bytes into the open stream (msw_core_gzip_append): uploaded, compressed by the same kernels."""
        data = bytes(data)
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._L.msw_core_gzip_append(self._h, data if data else None, len(data), C.byref(p), C.byref(n)))
        return C.string_at(p.value, n.value) if n.value else b""

    def gzip_end(self):
        """The final block, CRC-32 and length; closes the stream (msw_core_gzip_end)."""
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._L.msw_core_gzip_end(self._h, C.byref(p), C.byref(n)))
        return C.string_at(p.value, n.value) if n.value else b""

    def last_gzip_timing(self):
        """(device ms of the gzip kernels, bytes of text in, bytes out) of the stream open now or closed last"""
        ms, ni, no = C.c_double(), C.c_uint64(), C.c_uint64()
        self._check(self._L.msw_core_last_gzip_timing(self._h, C.byref(ms), C.byref(ni), C.byref(no)))
        return ms.value, ni.value, no.value

    # ---- --extract-reads: the records of a FASTQ file by read id (msw_fastq_*)
    def fastq_open(self, path):
        """A read file -- plain, gzip or BGZF -- resident on the device with its record index: a Fastq with .info
        (msw_fastq_info as a dict), .select(ids), .pieces(max_bytes), .pieces_gzip(max_bytes), .close().  A file outside
        the strict four-line grammar raises MswError naming the record."""
        h, info = C.c_void_p(), FastqInfo()
        self._check(self._L.msw_fastq_open(self._h, os.fsencode(path), C.byref(h), C.byref(info)))
        fq = Fastq(self, h, info.as_dict())
        self._fastqs.append(fq)
        return fq

    def last_fastq_timing(self):
        """(ms of the gather over the pieces since the last Fastq.select -- device events; the host clock under
        MSWEEP_HOST_EXTRACT=1 --, bytes gathered)"""
        ms, nb = C.c_double(), C.c_uint64()
        self._check(self._L.msw_fastq_last_timing(self._h, C.byref(ms), C.byref(nb)))
        return ms.value, nb.value

    # ---- gzip input inflated on the device (msw_core_inflate_gzip: the decoder's test and diagnostic entry)
    def inflate_gzip(self, data, chunk_bytes=0):
        """(text, info) of gzip bytes: inflated by the kernels -- chunk_bytes of payload per chunk, 0 the default -- or, where
        their result cannot be vouched for, by zlib; info is msw_inflate_info as a dict (on_device, reason, n_starts ...)."""
        data = bytes(data)
        p, n, info = C.c_void_p(), C.c_size_t(), InflateInfo()
        self._check(self._L.msw_core_inflate_gzip(self._h, data if data else None, len(data), int(chunk_bytes), C.byref(p), C.byref(n),
                                                  C.byref(info)))
        return (C.string_at(p.value, n.value) if n.value else b""), info.as_dict()

    def last_inflate(self):
        """One dict per file of the last read_alignment on this handle (msw_alignment_last_inflate): which path inflated
        each strand -- on_device, reason, chunks, starts, stage times; a plain file has only text_bytes."""
        n = C.c_size_t()
        self._check(self._L.msw_alignment_last_inflate(self._h, None, 0, C.byref(n)))
        infos = (InflateInfo * max(1, n.value))()
        self._check(self._L.msw_alignment_last_inflate(self._h, infos, n.value, C.byref(n)))
        return [infos[i].as_dict() for i in range(n.value)]

    def bin_reads(self, ec_rptr, ec_reads, targets, thresholds, want_reads=True):
        """mGEMS read binning of the last solve on the device (msw_core_bin_reads): the reads of EC j go to bin k when
        gamma(targets[k], j) >= log(thresholds[k]).  Returns (bin_ptr[n_targets + 1] uint64, reads uint32 or None,
        log_thr[n_targets]); bin k = reads[bin_ptr[k]:bin_ptr[k + 1]]."""
        ec_rptr = _arr(ec_rptr, np.uint64)
        ec_reads = _arr(ec_reads, np.uint32)
        if len(ec_rptr) == 0 or (len(ec_rptr) and int(ec_rptr[-1]) > len(ec_reads)):
            raise MswError("bin_reads: ec_rptr does not describe ec_reads")
        return self._bin(lambda t, th, n, bp, out, lt: self._L.msw_core_bin_reads(
            self._h, _ptr(ec_rptr), _ptr(ec_reads), len(ec_rptr) - 1, t, th, n, bp, out, lt), targets, thresholds, want_reads)

    def bin_reads_aln(self, aln, targets, thresholds, want_reads=True):
        """bin_reads on the classes of an alignment (msw_core_bin_reads_aln): a DeviceAlignment on this GPU is read
        where it lies."""
        return self._bin(lambda t, th, n, bp, out, lt: self._L.msw_core_bin_reads_aln(
            self._h, aln._h, t, th, n, bp, out, lt), targets, thresholds, want_reads)

    def _bin(self, call, targets, thresholds, want_reads):
        targets = _arr(targets, np.uint32)
        thresholds = _arr(thresholds, np.float64)
        if targets.shape != thresholds.shape or targets.ndim != 1:
            raise MswError("bin_reads: targets and thresholds must be 1-D arrays of one length")
        n = len(targets)
        bin_ptr = np.zeros(n + 1, np.uint64)
        log_thr = np.empty(n, np.float64)
        self._check(call(_ptr(targets), _ptr(thresholds), n, _ptr(bin_ptr), None, _ptr(log_thr)))
        if not want_reads:
            return bin_ptr, None, log_thr
        reads = np.empty(int(bin_ptr[-1]), np.uint32)
        self._check(call(_ptr(targets), _ptr(thresholds), n, _ptr(bin_ptr), _ptr(reads), None))
        return bin_ptr, reads, log_thr

    def assign_reads(self, ec_rptr, ec_reads, thresholds, targets, unassigned=True, keep_table=False, want_reads=True):
        """Every EC judged against ALL estimated groups (msw_core_assign_reads): pass(g, j) <=> gamma(g, j) >=
        log(thresholds[g]), thresholds for every group.  Returns a dict: bin_ptr (n_targets + 1 entries, one more with
        `unassigned`, whose last bin holds the reads no group claims), reads (or None), n_assigned[E] (groups that claim
        each EC) and class_reads (reads in ECs claimed by 0 / 1 / >= 2 groups).  keep_table: assign_table_* serve the
        read x target table of this call."""
        ec_rptr = _arr(ec_rptr, np.uint64)
        ec_reads = _arr(ec_reads, np.uint32)
        if len(ec_rptr) == 0 or int(ec_rptr[-1]) > len(ec_reads):
            raise MswError("assign_reads: ec_rptr does not describe ec_reads")
        return self._assign(lambda th, t, n, fl, bp, out, na, cl: self._L.msw_core_assign_reads(
            self._h, _ptr(ec_rptr), _ptr(ec_reads), len(ec_rptr) - 1, th, t, n, fl, bp, out, na, cl),
            len(ec_rptr) - 1, thresholds, targets, unassigned, keep_table, want_reads)

    def assign_reads_aln(self, aln, thresholds, targets, unassigned=True, keep_table=False, want_reads=True):
        """assign_reads on the classes of an alignment (msw_core_assign_reads_aln): a DeviceAlignment on this GPU is read
        where it lies."""
        return self._assign(lambda th, t, n, fl, bp, out, na, cl: self._L.msw_core_assign_reads_aln(
            self._h, aln._h, th, t, n, fl, bp, out, na, cl), int(aln.n_ecs), thresholds, targets, unassigned, keep_table,
            want_reads)

    def _assign(self, call, n_ecs, thresholds, targets, unassigned, keep_table, want_reads):
        thresholds = _arr(thresholds, np.float64)
        targets = _arr(targets, np.uint32)
        if thresholds.ndim != 1 or targets.ndim != 1:
            raise MswError("assign_reads: thresholds and targets must be 1-D arrays")
        if self.shape()[0] != len(thresholds):
            raise MswError("assign_reads: one threshold per estimated group")
        n = len(targets)
        flags = (ASSIGN_UNASSIGNED if unassigned else 0) | (ASSIGN_KEEP_TABLE if keep_table else 0)
        bin_ptr = np.zeros(n + 1 + (1 if unassigned else 0), np.uint64)
        n_assigned = np.zeros(max(int(n_ecs), 0), np.uint32)
        cls = np.zeros(3, np.uint64)
        reads = None
        if want_reads:      # the sizes first, then the fill: every call runs the whole pass
            self._check(call(_ptr(thresholds), _ptr(targets), n, flags & ~ASSIGN_KEEP_TABLE, _ptr(bin_ptr), None, None, None))
            reads = np.empty(int(bin_ptr[-1]), np.uint32)
        self._check(call(_ptr(thresholds), _ptr(targets), n, flags, _ptr(bin_ptr), _ptr(reads) if want_reads else None,
                         _ptr(n_assigned), _ptr(cls)))
        return dict(bin_ptr=bin_ptr, reads=reads, n_assigned=n_assigned, class_reads=cls)

    def assign_table_rows(self):
        """rows of the kept assignment table: the aligned reads (msw_core_assign_table_rows)"""
        n = C.c_size_t()
        self._check(self._L.msw_core_assign_table_rows(self._h, C.byref(n)))
        return n.value

    def assign_table_block(self, row_begin, row_end):
        """The rows [row_begin, row_end) of the kept assignment table as text formatted on the device
        (msw_core_assign_table_block): "id\t0\t1...\n" per aligned read, ascending id.  A copy of the bytes."""
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._L.msw_core_assign_table_block(self._h, int(row_begin), int(row_end), C.byref(p), C.byref(n)))
        return C.string_at(p.value, n.value) if n.value else b""

    def assign_table_block_gzip(self, row_begin, row_end, with_info=False):
        """assign_table_block into the open gzip stream (msw_core_assign_table_block_gzip): the compressed bytes and,
        with_info, the uncompressed length."""
        p, n, nt = C.c_void_p(), C.c_size_t(), C.c_size_t()
        self._check(self._L.msw_core_assign_table_block_gzip(self._h, int(row_begin), int(row_end), C.byref(p), C.byref(n),
                                                             C.byref(nt)))
        out = C.string_at(p.value, n.value) if n.value else b""
        return (out, nt.value) if with_info else out

    # ---- --write-read-probs: the probabilities at or above a threshold as sparse text (msw_core_sparse_probs_*)
    def sparse_probs(self, aln, threshold):
        """Selects the cells with gamma(g, j) >= log(threshold) of the last solve (msw_core_sparse_probs_begin): rows are
        ECs when aln is None, else the aligned reads of the alignment in ascending id.  Returns a SparseProbs with .rows,
        .log_threshold, .pieces(max_bytes), .pieces_gzip(max_bytes) and .last_timing()."""
        n, lt = C.c_uint64(), C.c_double()
        self._check(self._L.msw_core_sparse_probs_begin(self._h, aln._h if aln is not None else None, float(threshold),
                                                        C.byref(n), C.byref(lt)))
        return SparseProbs(self, n.value, lt.value)

    def set_trace_theta(self, n):
        self._check(self._L.msw_core_set_trace_theta(self._h, int(n)))

    def trace(self, n, with_theta=False):
        G, _, _ = self.shape()
        bound, nn, beta = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
        rs = np.full(n, -1, np.int32)
        th = np.full((n, G), np.nan) if with_theta else None
        got = C.c_size_t()
        self._check(self._L.msw_core_trace(self._h, n, _ptr(bound), _ptr(nn), _ptr(beta), _ptr(rs), _ptr(th),
                                           C.byref(got)))
        k = got.value
        return dict(n=k, bound=bound[:k], newnorm=nn[:k], beta=beta[:k], didreset=rs[:k],
                    theta=None if th is None else th[:k])

    # ---- bootstrap ------------------------------------------------------------------------
    def bootstrap(self, ec_counts, seed, bootstrap_count, rep_begin, rep_end, alpha0, tol=1e-6,
                  max_iters=5000, algo=ALGO_RCG, prec=PREC_DOUBLE):
        G, E, _ = self.shape()
        ec_counts = _arr(ec_counts, np.uint32)
        alpha0 = _arr(alpha0, np.float64)
        if len(ec_counts) != E or len(alpha0) != G:
            raise MswError("bootstrap: ec_counts / alpha0 length mismatch")
        n = int(rep_end) - int(rep_begin)
        theta = np.empty((max(n, 0), G))
        iters = np.zeros(max(n, 0), np.uint64)
        self._check(self._L.msw_core_bootstrap(self._h, _ptr(ec_counts), int(seed), int(bootstrap_count),
                                               int(rep_begin), int(rep_end), _ptr(alpha0), float(tol),
                                               int(max_iters), int(algo), int(prec), _ptr(theta), _ptr(iters)))
        return theta, iters

    def bootstrap_dist(self, comm, ec_counts, seed, bootstrap_count, n_replicates, alpha0, tol=1e-6,
                       max_iters=5000, algo=ALGO_RCG, prec=PREC_DOUBLE):
        """msw_core_bootstrap_dist: all replicates over the ranks of `comm`; every rank gets the whole
        n_replicates x G table (replicate order) and the iteration counts."""
        G, E, _ = self.shape()
        ec_counts = _arr(ec_counts, np.uint32)
        alpha0 = _arr(alpha0, np.float64)
        if len(ec_counts) != E or len(alpha0) != G:
            raise MswError("bootstrap_dist: ec_counts / alpha0 length mismatch")
        n = int(n_replicates)
        theta = np.empty((n, G))
        iters = np.zeros(n, np.uint64)
        self._check(self._L.msw_core_bootstrap_dist(self._h, comm._c, _ptr(ec_counts), int(seed),
                                                    int(bootstrap_count), n, _ptr(alpha0), float(tol),
                                                    int(max_iters), int(algo), int(prec), _ptr(theta), _ptr(iters)))
        return theta, iters

    def resample_counts(self, ec_counts, seed, bootstrap_count, rep_begin, rep_end):
        ec_counts = _arr(ec_counts, np.uint32)
        n = int(rep_end) - int(rep_begin)
        out = np.empty((max(n, 0), len(ec_counts)), np.uint32)
        self._check(self._L.msw_core_resample_counts(self._h, _ptr(ec_counts), len(ec_counts), int(seed),
                                                     int(bootstrap_count), int(rep_begin), int(rep_end),
                                                     _ptr(out)))
        return out

    # ---- EC-sharded solve -------------------------------------------------------------------
    def set_comm(self, comm):
        """Attach a communicator (Comm) -- this handle then holds one rank's block of ECs."""
        self._check(self._L.msw_core_set_comm(self._h, comm._c if comm is not None else None))
        self._comm = comm      # keep it alive

    # ---- measurement ------------------------------------------------------------------------
    def set_profiling(self, on):
        self._check(self._L.msw_core_set_profiling(self._h, int(bool(on))))

    def set_fixed_iters(self, on):
        self._check(self._L.msw_core_set_fixed_iters(self._h, int(bool(on))))

    def hbm_stream_rates(self, n_bytes=1 << 30, reps=5):
        """(read-only GB/s, triad GB/s) of this device on n_bytes of HBM: the practical ceiling (measurement only)."""
        r, t = C.c_double(), C.c_double()
        self._check(self._L.msw_core_hbm_stream_rates(self._h, int(n_bytes), int(reps), C.byref(r), C.byref(t)))
        return r.value, t.value

    def last_timing(self):
        t = Timing()
        self._check(self._L.msw_core_last_timing(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in Timing._fields_}

    def set_pack_schedule(self, enabled):
        """Order the cells of the NEXT likelihood for the LDS banks (default) or keep their CSR order (one solve only:
        the upload is faster than the iterations are slower).  msw_core_set_pack_schedule."""
        self._check(self._L.msw_core_set_pack_schedule(self._h, 1 if enabled else 0))

    def set_option(self, name, value):
        """msw_core_set_option: "check_every" n | "init_bound" b | "em_prior" 0 (MAP) / 1 (ML) | "em_stop" 0 (gain) /
        1 (largest move of a weight).  Persists on the handle."""
        if name not in _OPTS:
            raise MswError(f"set_option: unknown option `{name}`")
        self._check(self._L.msw_core_set_option(self._h, _OPTS[name], float(value)))

    def get_option(self, name):
        if name not in _OPTS:
            raise MswError(f"get_option: unknown option `{name}`")
        v = C.c_double()
        self._check(self._L.msw_core_get_option(self._h, _OPTS[name], C.byref(v)))
        return v.value

    def guarded_visits(self):
        """ECs pass B has taken through the cancellation guard since the likelihood became resident (all iterations)."""
        out = C.c_uint64(0)
        self._check(self._L.msw_core_guarded_visits(self._h, C.byref(out)))
        return int(out.value)

    def last_bootstrap_timing(self):
        t = BootstrapTiming()
        self._check(self._L.msw_core_last_bootstrap_timing(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in BootstrapTiming._fields_}


class Comm:
    """Communicator of the EC-sharded solve (include/msweep_core.h, "EC-sharded single solve")."""

    def __init__(self, c, owner=True):
        self._L = load_library()
        self._c = c
        self._owner = owner

    @staticmethod
    def unique_id():
        L = load_library()
        buf = (C.c_ubyte * 128)()
        if L.msw_comm_unique_id(buf) != 0:
            raise MswError(L.msw_comm_last_error().decode())
        return bytes(buf)

    @classmethod
    def rccl(cls, uid, rank, nranks, device):
        L = load_library()
        out = C.c_void_p()
        buf = (C.c_ubyte * 128).from_buffer_copy(uid)
        if L.msw_comm_create_rccl(buf, int(rank), int(nranks), int(device), C.byref(out)) != 0:
            raise MswError(L.msw_comm_last_error().decode())
        return cls(out)

    @classmethod
    def local(cls, nranks):
        """nranks communicators for nranks host threads of this process."""
        L = load_library()
        arr = (C.c_void_p * nranks)()
        if L.msw_comm_create_local(int(nranks), arr) != 0:
            raise MswError(L.msw_comm_last_error().decode())
        return [cls(C.c_void_p(arr[i])) for i in range(nranks)]

    @classmethod
    def shm(cls, name, rank, nranks, device=0):
        """Rank `rank` of `nranks` PROCESSES of this host meeting in the shared-memory segment `name` ("/...")."""
        L = load_library()
        out = C.c_void_p()
        if L.msw_comm_create_shm(name.encode(), int(rank), int(nranks), int(device), C.byref(out)) != 0:
            raise MswError(L.msw_comm_last_error().decode())
        return cls(out)

    def size(self):
        n, r = C.c_int(), C.c_int()
        if self._L.msw_comm_size(self._c, C.byref(n), C.byref(r)) != 0:
            raise MswError(self._L.msw_comm_last_error().decode())
        return n.value, r.value

    def rccl_count(self):
        """ncclCommCount of the communicator (0 for an in-process one)."""
        n = C.c_int()
        if self._L.msw_comm_rccl_count(self._c, C.byref(n)) != 0:
            raise MswError(self._L.msw_comm_last_error().decode())
        return n.value

    def allgather(self, send):
        """(nranks, len(send)) array: row r = rank r's `send` (host buffers; ncclAllGather underneath)."""
        send = _arr(send, np.float64).ravel()
        out = np.empty((self.size()[0], len(send)))
        if self._L.msw_comm_allgather(self._c, _ptr(send), len(send), _ptr(out)) != 0:
            raise MswError(self._L.msw_comm_last_error().decode())
        return out

    def allreduce(self, ints, reals, repeats=1):
        """Sums over the ranks of a uint64 and a float64 vector (msw_comm_allreduce); returns (ints, reals, ms per call)."""
        a = np.array(ints, np.uint64).ravel()
        b = np.array(reals, np.float64).ravel()
        ms = C.c_double()
        if self._L.msw_comm_allreduce(self._c, _ptr(a) if len(a) else None, len(a), _ptr(b) if len(b) else None, len(b),
                                      int(repeats), C.byref(ms)) != 0:
            raise MswError(self._L.msw_comm_last_error().decode())
        return a, b, ms.value

    def close(self):
        if self._c and self._owner:
            self._L.msw_comm_destroy(self._c)
        self._c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
