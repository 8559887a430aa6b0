"""ctypes mirror of include/tagdust_hip.h (the drop-in boundary for the reference's run_pHMM(),
src/barcode_hmm.h:342).  Fails loudly when the HIP library is missing or no MI355X is present."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TD_LIB_PATH", os.path.join(HERE, "libtagdust_hip.so"))   # TD_LIB_PATH: A/B another build

MODE_GET_LABEL = 1
MODE_GET_PROB = 4
MODE_ARCH_COMP = 5
MODE_RNA_DUST = 6      # run_rna_dust: -ref filter + DUST on reads as they were read; needs no model, no labels
NUM_OUTCOME_SLOTS = 8
NUM_BARCODE_BINS = 256
NUM_COUNTERS = NUM_OUTCOME_SLOTS + NUM_BARCODE_BINS
NUM_DIAG_COUNTERS = 64

# every symbol include/tagdust_hip.h declares
ABI_SYMBOLS = [
    "td_ctx_create", "td_ctx_destroy", "td_last_error", "td_logsum_table", "td_model_upload", "td_set_params",
    "td_batch_upload", "td_batch_upload_ascii", "td_run", "td_sync", "td_batch_download", "td_counts_reset",
    "td_counts_get", "td_diag_get", "td_counts_device_ptr", "td_last_kernel_ms", "td_timeline_origin", "td_last_kernel_times", "td_batch_info", "td_set_option", "td_get_option", "td_set_artifacts", "td_spec_source", "td_spec_prune_info", "td_spec_restart_info",
    "td_spec_probe", "td_spec_probe_params", "td_spec_wait",
    "td_submit", "td_wait", "td_host_alloc", "td_host_free", "td_set_batch_window", "td_set_window", "td_arch_scores",
    "td_artifact_hits_get",
]
MULTI_ABI_SYMBOLS = ["td_shard_bounds", "td_count_outcomes", "td_multi_create", "td_multi_destroy", "td_multi_last_error",
                     "td_multi_size", "td_multi_ctx", "td_multi_model_upload", "td_multi_set_params", "td_multi_set_window", "td_multi_set_artifacts",
                     "td_multi_decode", "td_multi_counts", "td_multi_counts_reset", "td_multi_uses_rccl", "td_bind_host_to_device", "td_host_halves_bench",
                     "td_multi_artifact_hits"]
IO_ABI_SYMBOLS = ["td_io_last_error", "td_reads_parse", "td_reads_free", "td_writer_open", "td_writer_write", "td_writer_close",
                  "td_fasta_parse", "td_fasta_free", "td_stream_run", "td_stream_survey", "td_stream_run_multi", "td_stream_run_multi_hits", "td_stream_release",
                  "td_format_q", "td_fingerprint_text", "td_writer_set_fingerprint_text"]
MODEL_ABI_SYMBOLS = ["td_arch_parse", "td_arch_free", "td_sequence_stats", "td_sequence_stats_window", "td_model_build", "td_model_tables_free",
                     "td_calibration_emit", "td_calibration_select", "td_calibration_free", "td_estimate_threshold",
                     "td_compare_architectures", "td_simreads", "td_text_free", "td_sequence_stats_limit",
                     "td_sequence_stats_device"]

# include/tagdust_run.h: the whole-run driver
RUN_ABI_SYMBOLS = ["td_run_opts_new", "td_run_opts_free", "td_run_last_error", "td_run_parse_args", "td_run_usage", "td_run_version",
                   "td_run_plan", "td_run_plan_free", "td_run_plan_describe", "td_run_output_files_describe", "td_run_arch_file_describe", "td_run_execute",
                   "td_run_report_clear", "td_run_format_summary"]

# include/tagdust_census.h: the census of barcode spellings
CENSUS_ABI_SYMBOLS = ["td_census_enable", "td_census_disable", "td_census_reset", "td_census_get", "td_census_host", "td_census_merge",
                      "td_census_key_text", "td_census_free"]
CENSUS_ENTRY_DTYPE = np.dtype([("key", "<u8"), ("count", "<i8")])
CENSUS_TOTALS = ("eligible", "counted", "skipped_empty", "skipped_long", "skipped_n", "overflow", "distinct")
CENSUS_DEFAULT_MASK = (1 << 1) | (1 << 3)   # EXTRACT_FAIL_ARCHITECTURE_MISMATCH, EXTRACT_FAIL_BAR_FINGER_NOT_FOUND
CENSUS_MAX_WORD = 28

# include/tagdust_samples.h: sample assignment by all 'B' segments
SAMPLES_ABI_SYMBOLS = ["td_samples_enable", "td_samples_disable", "td_samples_reset", "td_samples_get", "td_samples_name", "td_samples_key",
                       "td_samples_key_calls", "td_samples_host",
                       # ... and the join across input files
                       "td_samples_export_enable", "td_samples_export_disable", "td_samples_export_next", "td_samples_join_enable",
                       "td_samples_join_next", "td_samples_join_get", "td_samples_export_host", "td_samples_join_host"]
SAMPLES_TOTALS = ("eligible", "assigned", "unlisted", "incomplete", "overflow")
SAMPLES_PARTNER_FAILED = 0xFFFFFFFF   # the export word of a read that was not extracted
SAMPLES_MAX = 255
SAMPLES_MAX_SEGMENTS = 4
EXTRACT_SUCCESS = 0
EXTRACT_FAIL_BAR_FINGER_NOT_FOUND = 3

# include/tagdust_quality.h: the base-quality filter
QUALITY_ABI_SYMBOLS = ["td_qual_pack", "td_qual_host", "td_qual_enable", "td_qual_disable", "td_qual_reset", "td_qual_get", "td_qual_next"]
QUALITY_TOTALS = ("eligible", "passed", "failed", "low_bases")
QUAL_SEG_B = 1
QUAL_SEG_F = 2
EXTRACT_FAIL_LOW_BASE_QUALITY = 8    # TD_EXTRACT_FAIL_LOW_BASE_QUALITY (include/tagdust_hip.h): not an outcome of the reference

# include/tagdust_molecules.h: molecules per barcode
MOL_ABI_SYMBOLS = ["td_mol_enable", "td_mol_disable", "td_mol_reset", "td_mol_entries", "td_mol_get", "td_mol_summarise", "td_mol_host",
                   "td_mol_key", "td_mol_key_bin", "td_mol_dedup_enable", "td_mol_dedup_disable", "td_mol_dedup_get", "td_mol_dedup_host",
                   "td_mol_collapse_enable", "td_mol_collapse_disable", "td_mol_origins", "td_mol_collapse_get", "td_mol_collapse_entries",
                   "td_mol_host_origins", "td_mol_collapse_host", "td_mol_dedup_freeze", "td_mol_dedup_collapsed_host",
                   "td_mol_mate_enable", "td_mol_mate_disable", "td_mol_mate_next", "td_mol_host_mated", "td_mol_host_origins_mated",
                   "td_mol_dedup_host_mated", "td_mol_dedup_collapsed_host_mated",
                   "td_mol_mate_filter_enable", "td_mol_mate_filter_disable", "td_mol_mate_types"]
MOL_TOTALS = ("eligible", "counted", "skipped_empty", "skipped_n", "overflow", "molecules")
MOL_DEDUP_TOTALS = ("kept", "duplicates", "unjudged")
MOL_COLLAPSE_TOTALS = ("molecules_before", "molecules_after", "absorbed", "longest_chain")
MOL_ORIGIN_DTYPE = np.dtype([("w", "<u8"), ("fingerprint", "<i4"), ("n", "<i4")])   # td_mol_origin
EXTRACT_DUPLICATE = 7    # TD_EXTRACT_DUPLICATE (include/tagdust_hip.h): not an outcome of the reference
MOL_LEVELS = 10
MOL_ROW_DTYPE = np.dtype([("reads", "<i8"), ("molecules", "<i8"), ("levels", "<i8", (MOL_LEVELS,))])
MOL_DEFAULT_PREFIX = 20
MOL_DEFAULT_LOG2_SLOTS = 26

RESULT_DTYPE = np.dtype([
    ("f_score", "<f4"), ("b_score", "<f4"), ("r_score", "<f4"), ("bar_prob", "<f4"), ("mapq", "<f4"),
    ("read_type", "<i4"), ("barcode", "<i4"), ("fingerprint", "<i4"),
])


class TdError(RuntimeError):
    pass


class _Reads(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("text", C.c_void_p), ("name_off", C.POINTER(C.c_int64)),
                ("name_len", C.POINTER(C.c_int32)), ("qual_off", C.POINTER(C.c_int64)), ("offs", C.POINTER(C.c_int64)),
                ("codes", C.POINTER(C.c_uint8))]


class _Calibration(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("codes", C.POINTER(C.c_uint8)), ("offs", C.POINTER(C.c_int64)),
                ("is_random", C.POINTER(C.c_uint8)), ("scoring", C.c_void_p)]


class _SeqStats(C.Structure):
    _fields_ = [("background", C.c_double * 5), ("expected_5_len", C.c_double), ("expected_3_len", C.c_double),
                ("mean_5_len", C.c_double), ("stdev_5_len", C.c_double), ("mean_3_len", C.c_double),
                ("stdev_3_len", C.c_double), ("average_length", C.c_double), ("max_seq_len", C.c_int32)]


class _ModelDesc(C.Structure):
    _fields_ = [
        ("S", C.c_int32), ("H", C.c_int32), ("C", C.c_int32), ("avg_len", C.c_int32), ("bg", C.c_float * 5),
        ("n_hmm", C.c_void_p), ("n_col", C.c_void_p), ("skip", C.c_void_p), ("seg_type", C.c_void_p),
        ("finger_len", C.c_void_p), ("trans", C.c_void_p), ("eM", C.c_void_p), ("eI", C.c_void_p),
        ("sM", C.c_void_p), ("sI", C.c_void_p), ("label", C.c_void_p), ("A", C.c_void_p),
    ]


_lib = None


def load_library():
    """dlopen libtagdust_hip.so (no GPU needed for this step)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TdError("%s is missing: run `python -m tagdust_amd.build` (or __graft_entry__.build()); "
                      "there is no CPU fallback" % LIB_PATH)
    if "TD_LIB_PATH" not in os.environ:
        try:   # a library older than its sources measures / tests the wrong code: say so (the GPU box only has the prebuilt file)
            from . import build as _b
            if _b.needs_build():
                import sys
                sys.stderr.write("tagdust_amd: %s is older than its sources -- run `python -m tagdust_amd.build`\n" % LIB_PATH)
        except Exception:
            pass
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # read by the HIP runtime at its first call (td_want_hw_queues, td_api.hip)
    lib = C.CDLL(LIB_PATH)
    lib.td_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.td_ctx_destroy.argtypes = [C.c_void_p]
    lib.td_ctx_destroy.restype = None
    lib.td_last_error.argtypes = [C.c_void_p]
    lib.td_last_error.restype = C.c_char_p
    lib.td_logsum_table.restype = C.POINTER(C.c_float)
    lib.td_model_upload.argtypes = [C.c_void_p, C.POINTER(_ModelDesc)]
    lib.td_set_params.argtypes = [C.c_void_p, C.c_float, C.c_int32, C.c_int32]
    lib.td_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
    if hasattr(lib, "td_set_artifacts"):
        lib.td_set_artifacts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    if hasattr(lib, "td_get_option"):   # absent from older builds loaded through TD_LIB_PATH for A/B runs
        lib.td_get_option.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int32)]
    lib.td_spec_source.argtypes = [C.POINTER(_ModelDesc), C.c_char_p, C.c_int64]
    lib.td_spec_source.restype = C.c_int64
    lib.td_spec_prune_info.argtypes = [C.POINTER(_ModelDesc), C.c_int32, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.td_batch_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.td_batch_upload_ascii.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.td_run.argtypes = [C.c_void_p, C.c_int]
    lib.td_sync.argtypes = [C.c_void_p]
    lib.td_batch_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.td_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.POINTER(C.c_int64)]
    lib.td_wait.argtypes = [C.c_void_p, C.c_int64]
    lib.td_host_alloc.argtypes = [C.c_size_t]
    lib.td_host_alloc.restype = C.c_void_p
    lib.td_host_free.argtypes = [C.c_void_p]
    lib.td_host_free.restype = None
    lib.td_set_batch_window.argtypes = [C.c_void_p, C.c_int64, C.c_int64]
    lib.td_set_window.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.td_arch_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.td_shard_bounds.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.td_shard_bounds.restype = None
    lib.td_count_outcomes.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.td_count_outcomes.restype = None
    lib.td_multi_create.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    lib.td_multi_destroy.argtypes = [C.c_void_p]
    lib.td_multi_destroy.restype = None
    lib.td_multi_last_error.argtypes = [C.c_void_p]
    lib.td_multi_last_error.restype = C.c_char_p
    lib.td_multi_size.argtypes = [C.c_void_p]
    lib.td_multi_ctx.argtypes = [C.c_void_p, C.c_int32]
    lib.td_multi_ctx.restype = C.c_void_p
    lib.td_multi_model_upload.argtypes = [C.c_void_p, C.POINTER(_ModelDesc)]
    lib.td_multi_set_params.argtypes = [C.c_void_p, C.c_float, C.c_int32, C.c_int32]
    lib.td_multi_set_window.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.td_multi_set_artifacts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    lib.td_multi_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.td_multi_counts.argtypes = [C.c_void_p, C.c_void_p]
    lib.td_multi_counts_reset.argtypes = [C.c_void_p]
    lib.td_multi_uses_rccl.argtypes = [C.c_void_p]
    if hasattr(lib, "td_bind_host_to_device"):
        lib.td_bind_host_to_device.argtypes = [C.c_int32]
        lib.td_bind_host_to_device.restype = C.c_int32
    lib.td_counts_reset.argtypes = [C.c_void_p]
    lib.td_counts_get.argtypes = [C.c_void_p, C.c_void_p]
    if hasattr(lib, "td_diag_get"):
        lib.td_diag_get.argtypes = [C.c_void_p, C.c_void_p]
    lib.td_counts_device_ptr.argtypes = [C.c_void_p]
    lib.td_counts_device_ptr.restype = C.c_void_p
    lib.td_last_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    if hasattr(lib, "td_timeline_origin"):
        lib.td_timeline_origin.argtypes = [C.c_void_p]
        lib.td_last_kernel_times.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int32)]
    lib.td_batch_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    lib.td_arch_parse.argtypes = [C.POINTER(C.c_char_p), C.c_int32, C.POINTER(C.c_void_p)]
    lib.td_arch_free.argtypes = [C.c_void_p]
    lib.td_arch_free.restype = None
    lib.td_sequence_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(_SeqStats)]
    lib.td_sequence_stats_window.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.POINTER(_SeqStats)]
    lib.td_sequence_stats_limit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.POINTER(_SeqStats)]
    lib.td_sequence_stats_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                             C.POINTER(_SeqStats)]
    lib.td_artifact_hits_get.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    lib.td_multi_artifact_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    lib.td_model_build.argtypes = [C.c_void_p, C.POINTER(_SeqStats), C.c_float, C.c_float, C.POINTER(C.c_void_p)]
    lib.td_model_tables_free.argtypes = [C.c_void_p]
    lib.td_model_tables_free.restype = None
    lib.td_calibration_emit.argtypes = [C.c_void_p, C.POINTER(_SeqStats), C.c_float, C.c_uint32, C.c_int32, C.c_int32,
                                        C.POINTER(C.POINTER(_Calibration))]
    lib.td_calibration_select.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.td_calibration_select.restype = C.c_float
    lib.td_calibration_free.argtypes = [C.POINTER(_Calibration)]
    lib.td_calibration_free.restype = None
    lib.td_estimate_threshold.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_SeqStats), C.c_float, C.c_uint32, C.c_int32, C.c_int32,
                                          C.POINTER(C.c_float)]
    lib.td_compare_architectures.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                             C.c_float, C.c_float, C.c_int32, C.c_void_p, C.POINTER(C.c_int32)]
    lib.td_reads_parse.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.POINTER(_Reads))]
    lib.td_reads_free.argtypes = [C.POINTER(_Reads)]
    lib.td_reads_free.restype = None
    lib.td_writer_open.argtypes = [C.c_char_p, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.td_writer_write.argtypes = [C.c_void_p, C.POINTER(_Reads), C.c_void_p, C.c_void_p]
    lib.td_writer_close.argtypes = [C.c_void_p]
    _lib = lib
    return lib


def make_model_desc(md):
    """Build the C td_model_desc from a mapping of numpy tables; returns (desc, arrays to keep alive)."""
    S, H, Cc = int(md["S"]), int(md["H"]), int(md["C"])
    a = {
        "n_hmm": np.ascontiguousarray(md["n_hmm"], np.int32), "n_col": np.ascontiguousarray(md["n_col"], np.int32),
        "skip": np.ascontiguousarray(md["skip"], np.float32),
        "seg_type": np.ascontiguousarray(md["seg_type"], np.int32).astype(np.int8),
        "finger_len": np.where(np.asarray(md["seg_type"]) == ord("F"), np.asarray(md["seg_len"]), 0).astype(np.int32),
        "trans": np.ascontiguousarray(md["trans"], np.float32).reshape(Cc, 9),
        "eM": np.ascontiguousarray(md["eM"], np.float32).reshape(Cc, 5),
        "eI": np.ascontiguousarray(md["eI"], np.float32).reshape(Cc, 5),
        "sM": np.ascontiguousarray(md["sM"], np.float32).reshape(Cc),
        "sI": np.ascontiguousarray(md["sI"], np.float32).reshape(Cc),
        "label": np.ascontiguousarray(md["label"], np.int32).reshape(H),
        "A": np.ascontiguousarray(md["A"], np.float32).reshape(H, H),
    }
    d = _ModelDesc()
    d.S, d.H, d.C, d.avg_len = S, H, Cc, int(md["avg_len"])
    for i in range(5):
        d.bg[i] = float(np.float32(md["bg"][i]))
    for k, v in a.items():
        setattr(d, k, v.ctypes.data)
    return d, a


def build_model(segments, codes, offs, e=0.05, d=0.1, stats_override=None, window=None):
    """Host model construction through the C library (include/tagdust_model.h; no GPU needed):
    td_arch_parse -> td_sequence_stats -> td_model_build.  segments: ["B:ACGT,...", "R:N", ...].
    Returns (model mapping with the golden-fixture keys, stats dict)."""
    lib = load_library()
    arr = (C.c_char_p * len(segments))(*[s.encode() for s in segments])
    arch = C.c_void_p()
    if lib.td_arch_parse(arr, len(segments), C.byref(arch)) != 0:
        raise TdError("td_arch_parse failed for %r" % (segments,))
    try:
        codes = np.ascontiguousarray(codes, np.uint8)
        offs = np.ascontiguousarray(offs, np.int64)
        st = _SeqStats()
        ms, me = window if window else (-1, -1)
        if lib.td_sequence_stats_window(arch, codes.ctypes.data, offs.ctypes.data, len(offs) - 1, int(ms), int(me), C.byref(st)) != 0:
            raise TdError("td_sequence_stats failed")
        if stats_override:
            for k, v in stats_override.items():
                setattr(st, k, v)
        tab = C.c_void_p()
        if lib.td_model_build(arch, C.byref(st), float(e), float(d), C.byref(tab)) != 0:
            raise TdError("td_model_build failed")
        try:
            desc = C.cast(tab, C.POINTER(_ModelDesc)).contents
            S, H, Cc = desc.S, desc.H, desc.C

            def arr_of(ptr, ctype, n, dtype):
                return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n,)).astype(dtype).copy()
            md = {
                "S": S, "H": H, "C": Cc, "avg_len": desc.avg_len, "bg": np.array(list(desc.bg), np.float32),
                "n_hmm": arr_of(desc.n_hmm, C.c_int32, S, np.int32), "n_col": arr_of(desc.n_col, C.c_int32, S, np.int32),
                "skip": arr_of(desc.skip, C.c_float, S, np.float32),
                "seg_type": arr_of(desc.seg_type, C.c_int8, S, np.int32),
                "trans": arr_of(desc.trans, C.c_float, Cc * 9, np.float32).reshape(Cc, 9),
                "eM": arr_of(desc.eM, C.c_float, Cc * 5, np.float32).reshape(Cc, 5),
                "eI": arr_of(desc.eI, C.c_float, Cc * 5, np.float32).reshape(Cc, 5),
                "sM": arr_of(desc.sM, C.c_float, Cc, np.float32), "sI": arr_of(desc.sI, C.c_float, Cc, np.float32),
                "label": arr_of(desc.label, C.c_int32, H, np.int32),
                "A": arr_of(desc.A, C.c_float, H * H, np.float32).reshape(H, H),
            }
            fl = arr_of(desc.finger_len, C.c_int32, S, np.int32)
            md["seg_len"] = np.where(md["seg_type"] == ord("F"), fl, md["n_col"]).astype(np.int32)
            stats = {k: (list(getattr(st, k)) if k == "background" else getattr(st, k)) for k, _ in _SeqStats._fields_}
            return md, stats
        finally:
            lib.td_model_tables_free(tab)
    finally:
        lib.td_arch_free(arch)


def _arch_and_stats(lib, segments, codes, offs):
    arr = (C.c_char_p * len(segments))(*[s.encode() for s in segments])
    arch = C.c_void_p()
    if lib.td_arch_parse(arr, len(segments), C.byref(arch)) != 0:
        raise TdError("td_arch_parse failed for %r" % (segments,))
    codes = np.ascontiguousarray(codes, np.uint8)
    offs = np.ascontiguousarray(offs, np.int64)
    st = _SeqStats()
    if lib.td_sequence_stats(arch, codes.ctypes.data, offs.ctypes.data, len(offs) - 1, C.byref(st)) != 0:
        lib.td_arch_free(arch)
        raise TdError("td_sequence_stats failed")
    return arch, st


def _parse_arch(lib, segments):
    arr = (C.c_char_p * len(segments))(*[s.encode() for s in segments])
    arch = C.c_void_p()
    if lib.td_arch_parse(arr, len(segments), C.byref(arch)) != 0:
        raise TdError("td_arch_parse failed for %r" % (segments,))
    return arch


def sequence_stats(segments, codes, offs, scan_limit=1000001, window=None):
    """td_sequence_stats_limit on the host (no GPU needed): the _SeqStats structure itself, so that two results can be
    compared as bytes."""
    lib = load_library()
    arch = _parse_arch(lib, segments)
    try:
        codes = np.ascontiguousarray(codes, np.uint8)
        offs = np.ascontiguousarray(offs, np.int64)
        ms, me = window if window else (-1, -1)
        st = _SeqStats()
        if lib.td_sequence_stats_limit(arch, codes.ctypes.data, offs.ctypes.data, len(offs) - 1, int(scan_limit), int(ms), int(me),
                                       C.byref(st)) != 0:
            raise TdError("td_sequence_stats_limit failed")
        return st
    finally:
        lib.td_arch_free(arch)


def sequence_stats_device(ctx, segments, codes, offs, scan_limit=1000001, window=None):
    """td_sequence_stats_device: the same statistics with the counting on ctx's device."""
    lib = load_library()
    arch = _parse_arch(lib, segments)
    try:
        codes = np.ascontiguousarray(codes, np.uint8)
        offs = np.ascontiguousarray(offs, np.int64)
        ms, me = window if window else (-1, -1)
        st = _SeqStats()
        if lib.td_sequence_stats_device(ctx.h, arch, codes.ctypes.data, offs.ctypes.data, len(offs) - 1, int(scan_limit), int(ms), int(me),
                                        C.byref(st)) != 0:
            raise TdError(lib.td_last_error(ctx.h).decode() or "td_sequence_stats_device failed")
        return st
    finally:
        lib.td_arch_free(arch)


def calibration_emit(segments, codes, offs, d=0.1, seed=42, n_reads=400000, rng=0):
    """The simulated reads of the reference's threshold calibration (calibrateQ.c:88-113) for this architecture and
    these sequence statistics: returns (codes, offs, is_random)."""
    lib = load_library()
    arch, st = _arch_and_stats(lib, segments, codes, offs)
    try:
        p = C.POINTER(_Calibration)()
        if lib.td_calibration_emit(arch, C.byref(st), float(d), int(seed), int(n_reads), int(rng), C.byref(p)) != 0:
            raise TdError("td_calibration_emit failed")
        c = p.contents
        n = int(c.n_reads)
        o = np.ctypeslib.as_array(c.offs, shape=(n + 1,)).copy()
        out = (np.ctypeslib.as_array(c.codes, shape=(int(o[-1]),)).copy(), o, np.ctypeslib.as_array(c.is_random, shape=(n,)).copy())
        lib.td_calibration_free(p)
        return out
    finally:
        lib.td_arch_free(arch)


def calibration_select(mapq, is_random):
    lib = load_library()
    q = np.ascontiguousarray(mapq, np.float32)
    r = np.ascontiguousarray(is_random, np.uint8)
    return float(np.float32(lib.td_calibration_select(q.ctypes.data, r.ctypes.data, len(q))))


def estimate_threshold(ctx, segments, codes, offs, d=0.1, seed=42, n_reads=400000, rng=0):
    """estimateQthreshold() with the scoring on the GPU (TD_MODE_GET_PROB)."""
    lib = load_library()
    arch, st = _arch_and_stats(lib, segments, codes, offs)
    try:
        thr = C.c_float()
        if lib.td_estimate_threshold(ctx.h, arch, C.byref(st), float(d), int(seed), int(n_reads), int(rng), C.byref(thr)) != 0:
            raise TdError(lib.td_last_error(ctx.h).decode() or "td_estimate_threshold failed")
        return float(np.float32(thr.value))
    finally:
        lib.td_arch_free(arch)


def compare_architectures(ctx, candidates, codes, offs, e=0.05, d=0.1, n_threads=8):
    """test_architectures(): candidates = list of segment-string lists; returns (posteriors float32[n], best index)."""
    lib = load_library()
    handles = []
    try:
        for segs in candidates:
            arr = (C.c_char_p * len(segs))(*[s.encode() for s in segs])
            h = C.c_void_p()
            if lib.td_arch_parse(arr, len(segs), C.byref(h)) != 0:
                raise TdError("td_arch_parse failed for %r" % (segs,))
            handles.append(h)
        arr = (C.c_void_p * len(handles))(*[h.value for h in handles])
        codes = np.ascontiguousarray(codes, np.uint8)
        offs = np.ascontiguousarray(offs, np.int64)
        post = np.zeros(len(handles), np.float32)
        best = C.c_int32(-1)
        if lib.td_compare_architectures(ctx.h, arr, len(handles), codes.ctypes.data, offs.ctypes.data, len(offs) - 1,
                                        float(e), float(d), int(n_threads), post.ctypes.data, C.byref(best)) != 0:
            raise TdError(lib.td_last_error(ctx.h).decode() or "td_compare_architectures failed")
        return post, int(best.value)
    finally:
        for h in handles:
            lib.td_arch_free(h)


class _Fasta(C.Structure):
    _fields_ = [("n_seq", C.c_int32), ("string", C.POINTER(C.c_uint8)), ("s_index", C.POINTER(C.c_int32)),
                ("names", C.POINTER(C.c_char_p))]


def parse_fasta(text):
    """-ref artifact sequences as read_fasta() (src/io.c:1912-2001) stores them: (string uint8, s_index int32, names)."""
    lib = load_library()
    buf = np.frombuffer(bytes(text), dtype=np.uint8)
    p = C.POINTER(_Fasta)()
    lib.td_fasta_parse.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    lib.td_fasta_free.argtypes = [C.c_void_p]
    if lib.td_fasta_parse(buf.ctypes.data, len(buf), C.byref(p)) != 0:
        raise TdError("td_fasta_parse failed")
    try:
        f = p.contents
        n = int(f.n_seq)
        ix = np.ctypeslib.as_array(f.s_index, shape=(n + 1,)).copy()
        st = np.ctypeslib.as_array(f.string, shape=(max(int(ix[-1]), 1),))[:int(ix[-1])].copy()
        names = [f.names[j] for j in range(n)]
    finally:
        lib.td_fasta_free(p)
    return st, ix, names


class ParsedReads:
    """FASTQ/FASTA text parsed by the library (include/tagdust_io.h); keeps the text buffer alive."""

    def __init__(self, text, n_threads=0):
        lib = load_library()
        self._buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, np.uint8)
        self._p = C.POINTER(_Reads)()
        if lib.td_reads_parse(self._buf.ctypes.data, len(self._buf), int(n_threads), C.byref(self._p)) != 0:
            self._p = None
            lib.td_io_last_error.restype = C.c_char_p
            raise TdError(lib.td_io_last_error().decode() or "td_reads_parse failed")
        r = self._p.contents
        self.n = int(r.n_reads)
        self.offs = np.ctypeslib.as_array(r.offs, shape=(self.n + 1,)).copy()
        self.codes = np.ctypeslib.as_array(r.codes, shape=(max(int(self.offs[-1]), 1),))[:int(self.offs[-1])].copy()
        self.name_off = np.ctypeslib.as_array(r.name_off, shape=(max(self.n, 1),))[:self.n].copy()
        self.name_len = np.ctypeslib.as_array(r.name_len, shape=(max(self.n, 1),))[:self.n].copy()
        self.qual_off = np.ctypeslib.as_array(r.qual_off, shape=(max(self.n, 1),))[:self.n].copy()

    def names(self):
        b = self._buf.tobytes()
        return [b[o:o + l] for o, l in zip(self.name_off, self.name_len)]

    def close(self):
        if self._p:
            load_library().td_reads_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fingerprint_text(fingerprint):
    """td_fingerprint_text: the bases a fingerprint stands for, as the reference's get_finger_seq gives them."""
    lib = load_library()
    lib.td_fingerprint_text.argtypes = [C.c_int32, C.c_char_p]
    buf = C.create_string_buffer(256)
    n = lib.td_fingerprint_text(int(fingerprint), buf)
    assert n == len(buf.value)
    return buf.value.decode()


def write_demultiplexed(prefix, segments, reads, res, seq_out, fingerprint_text=False):
    """print_all() for one input file through the library: res (RESULT_DTYPE) and seq_out as td_batch_download gives them.
    fingerprint_text: td_writer_set_fingerprint_text, ";FP:ACGT" instead of ";FP:27"."""
    lib = load_library()
    lib.td_writer_set_fingerprint_text.argtypes = [C.c_void_p, C.c_int]
    arr = (C.c_char_p * len(segments))(*[s.encode() for s in segments])
    arch = C.c_void_p()
    if lib.td_arch_parse(arr, len(segments), C.byref(arch)) != 0:
        raise TdError("td_arch_parse failed")
    try:
        w = C.c_void_p()
        if lib.td_writer_open(prefix.encode(), arch, C.byref(w)) != 0:
            raise TdError("td_writer_open failed for %s" % prefix)
        if lib.td_writer_set_fingerprint_text(w, 1 if fingerprint_text else 0) != 0:
            raise TdError("td_writer_set_fingerprint_text failed")
        res = np.ascontiguousarray(res, RESULT_DTYPE)
        seq_out = np.ascontiguousarray(seq_out, np.uint8)
        rc = lib.td_writer_write(w, reads._p, res.ctypes.data, seq_out.ctypes.data)
        rc |= lib.td_writer_close(w)
        if rc != 0:
            raise TdError("td_writer_write/close failed")
    finally:
        lib.td_arch_free(arch)


class _StreamOpts(C.Structure):
    _fields_ = [("batch_reads", C.c_int32), ("n_threads", C.c_int32), ("block_bytes", C.c_int64), ("fingerprint_text", C.c_int32)]


class _StreamStats(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("n_batches", C.c_int64), ("bytes_in", C.c_int64), ("bytes_out", C.c_int64),
                ("wall_s", C.c_double), ("read_s", C.c_double), ("parse_s", C.c_double), ("decode_s", C.c_double),
                ("write_s", C.c_double), ("codes_fnv", C.c_uint64)]


def stream_run(ctx, in_path, segments=None, out_prefix=None, batch_reads=0, n_threads=0, block_bytes=0, fingerprint_text=False):
    """td_stream_run: one input file through parse -> decode -> write as a pipeline; ctx None = parse-only run (no GPU).
    Returns the statistics as a dict."""
    lib = load_library()
    lib.td_stream_run.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_char_p, C.POINTER(_StreamOpts), C.POINTER(_StreamStats)]
    lib.td_io_last_error.restype = C.c_char_p
    arch = C.c_void_p()
    if segments is not None:
        arr = (C.c_char_p * len(segments))(*[s.encode() for s in segments])
        if lib.td_arch_parse(arr, len(segments), C.byref(arch)) != 0:
            raise TdError("td_arch_parse failed for %r" % (segments,))
    try:
        o = _StreamOpts(int(batch_reads), int(n_threads), int(block_bytes), 1 if fingerprint_text else 0)
        st = _StreamStats()
        rc = lib.td_stream_run(ctx.h if ctx is not None else None, os.fsencode(in_path), arch if segments is not None else None,
                               os.fsencode(out_prefix) if out_prefix is not None else None, C.byref(o), C.byref(st))
        if rc != 0:
            raise TdError(lib.td_io_last_error().decode() or "td_stream_run failed")
        return {k: getattr(st, k) for k, _ in _StreamStats._fields_}
    finally:
        if arch:
            lib.td_arch_free(arch)


def stream_survey(ctx, in_path, batch_reads=0, n_threads=0, block_bytes=0):
    """td_stream_survey: one input file through parse -> decode, nothing written; what the context accumulates is the result.
    Returns the statistics as a dict."""
    lib = load_library()
    lib.td_stream_survey.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(_StreamOpts), C.POINTER(_StreamStats)]
    lib.td_io_last_error.restype = C.c_char_p
    o = _StreamOpts(int(batch_reads), int(n_threads), int(block_bytes), 0)
    st = _StreamStats()
    if lib.td_stream_survey(ctx.h, os.fsencode(in_path), C.byref(o), C.byref(st)) != 0:
        raise TdError(lib.td_io_last_error().decode() or "td_stream_survey failed")
    return {k: getattr(st, k) for k, _ in _StreamStats._fields_}


class _StreamFile(C.Structure):
    _fields_ = [("path", C.c_char_p), ("arch", C.c_void_p), ("ctx", C.POINTER(C.c_void_p))]


def stream_run_multi(files, out_prefix, n_devices=1, dust=100, batch_reads=0, n_threads=0, block_bytes=0, fingerprint_text=False):
    """td_stream_run_multi: the input files of one paired / multi-read run in lock-step.  files: a list of
    (path, segments, contexts) -- contexts = one TagdustHip per device holding that file's model and parameters.  A file whose
    architecture is a single read segment ("R:N") is not decoded but goes through run_rna_dust: with contexts (no model needed;
    their dust must equal `dust`) on the devices, TD_MODE_RNA_DUST; with None on the host.  A -ref artifact filter
    (set_artifacts) set on any file's contexts must be set on every file's, so that every file needs contexts then; batch_reads
    defaults to the reference's 1 000 001 records with a filter.  Returns (statistics dict, counters int64[264])."""
    lib = load_library()
    lib.td_stream_run_multi.argtypes = [C.POINTER(_StreamFile), C.c_int32, C.c_int32, C.c_char_p, C.c_int32, C.POINTER(_StreamOpts),
                                        C.POINTER(_StreamStats), C.c_void_p]
    lib.td_io_last_error.restype = C.c_char_p
    arr = (_StreamFile * len(files))()
    archs, keep = [], []
    try:
        for k, (path, segments, ctxs) in enumerate(files):
            a = C.c_void_p()
            sa = (C.c_char_p * len(segments))(*[s.encode() for s in segments])
            if lib.td_arch_parse(sa, len(segments), C.byref(a)) != 0:
                raise TdError("td_arch_parse failed for %r" % (segments,))
            archs.append(a)
            arr[k].path = os.fsencode(path)
            arr[k].arch = a
            if ctxs is not None:
                if len(ctxs) != n_devices:
                    raise TdError("stream_run_multi: %d contexts for %d devices" % (len(ctxs), n_devices))
                cp = (C.c_void_p * n_devices)(*[c.h for c in ctxs])
                keep.append(cp)
                arr[k].ctx = C.cast(cp, C.POINTER(C.c_void_p))
        o = _StreamOpts(int(batch_reads), int(n_threads), int(block_bytes), 1 if fingerprint_text else 0)
        st = _StreamStats()
        counts = np.zeros(264, np.int64)
        rc = lib.td_stream_run_multi(arr, len(files), int(n_devices), os.fsencode(out_prefix), int(dust), C.byref(o), C.byref(st), counts.ctypes.data)
        if rc != 0:
            raise TdError(lib.td_io_last_error().decode() or "td_stream_run_multi failed")
        return {k: getattr(st, k) for k, _ in _StreamStats._fields_}, counts
    finally:
        for a in archs:
            if a:
                lib.td_arch_free(a)


class _RunOpts(C.Structure):
    """td_run_opts (include/tagdust_run.h)"""
    _fields_ = [("segments", C.c_char_p * 10), ("arch_file", C.c_char_p), ("outfile", C.c_char_p), ("num_threads", C.c_int32),
                ("confidence_threshold", C.c_float), ("sequencer_error_rate", C.c_float), ("indel_frequency", C.c_float),
                ("minlen", C.c_int32), ("dust", C.c_int32), ("reference_fasta", C.c_char_p), ("filter_error", C.c_int32),
                ("matchstart", C.c_int32), ("matchend", C.c_int32), ("seed", C.c_uint32), ("n_infiles", C.c_int32),
                ("infile", C.POINTER(C.c_char_p)), ("n_devices", C.c_int32), ("devices", C.c_int32 * 16), ("flavour", C.c_int32),
                ("host_threads", C.c_int32), ("batch_reads", C.c_int32), ("sync_compile", C.c_int32), ("stats_on_host", C.c_int32),
                ("force", C.c_int32), ("dry_run", C.c_int32), ("help", C.c_int32), ("version", C.c_int32), ("echo_log", C.c_int32),
                ("argc", C.c_int32), ("argv", C.POINTER(C.c_char_p)), ("unknown_barcodes", C.c_int32), ("unknown_slots_log2", C.c_int32),
                ("fingerprint_seq", C.c_int32), ("molecules", C.c_int32), ("molecules_prefix", C.c_int32), ("molecules_slots_log2", C.c_int32),
                ("dedup", C.c_int32), ("collapse_umis", C.c_int32), ("dedup_collapsed", C.c_int32)]


class _RunOptsMate(C.Structure):
    """td_run_opts (include/tagdust_run.h) as it is now: _RunOpts -- whose last field tests/test_dedup_collapsed.py pins -- and the
    field appended behind it; this is the structure every td_run_* call is given"""
    _fields_ = _RunOpts._fields_ + [("mate_bases", C.c_int32), ("mate_filter", C.c_int32)]


class _RunOptsSamples(C.Structure):
    """td_run_opts as it is now: _RunOptsMate -- whose last fields tests/test_mate_filter.py pins -- and the field appended behind it;
    this is the structure every td_run_* call is given"""
    _fields_ = _RunOptsMate._fields_ + [("samples_file", C.c_char_p)]


class _RunOptsQuality(C.Structure):
    """td_run_opts as it is now: _RunOptsSamples -- whose last field tests/test_samples.py pins -- and the fields appended behind it;
    this is the structure every td_run_* call is given"""
    _fields_ = _RunOptsSamples._fields_ + [("min_base_quality", C.c_int32), ("max_low_bases", C.c_int32), ("quality_segments", C.c_int32),
                                           ("quality_offset", C.c_int32)]


class _CensusTotals(C.Structure):
    """td_census_totals (include/tagdust_census.h)"""
    _fields_ = [(f, C.c_int64) for f in CENSUS_TOTALS]

    def as_dict(self):
        return {f: int(getattr(self, f)) for f in CENSUS_TOTALS}


class _SamplesTotals(C.Structure):
    """td_samples_totals (include/tagdust_samples.h)"""
    _fields_ = [(f, C.c_int64) for f in SAMPLES_TOTALS]

    def as_dict(self):
        return {f: int(getattr(self, f)) for f in SAMPLES_TOTALS}


class _SamplesJoinTotals(C.Structure):
    """td_samples_join_totals (include/tagdust_samples.h)"""
    _fields_ = [("t", _SamplesTotals), ("partner_failed", C.c_int64)]

    def as_dict(self):
        return dict(self.t.as_dict(), partner_failed=int(self.partner_failed))


class _QualParams(C.Structure):
    """td_qual_params (include/tagdust_quality.h)"""
    _fields_ = [("min_quality", C.c_int32), ("offset", C.c_int32), ("max_low", C.c_int32), ("segments", C.c_int32)]


class _QualTotals(C.Structure):
    """td_qual_totals (include/tagdust_quality.h)"""
    _fields_ = [(f, C.c_int64) for f in QUALITY_TOTALS]

    def as_dict(self):
        return {f: int(getattr(self, f)) for f in QUALITY_TOTALS}


class _MolTotals(C.Structure):
    """td_mol_totals (include/tagdust_molecules.h)"""
    _fields_ = [(f, C.c_int64) for f in MOL_TOTALS]

    def as_dict(self):
        return {f: int(getattr(self, f)) for f in MOL_TOTALS}


class _MolDedupTotals(C.Structure):
    """td_mol_dedup_totals (include/tagdust_molecules.h)"""
    _fields_ = [(f, C.c_int64) for f in MOL_DEDUP_TOTALS]

    def as_dict(self):
        return {f: int(getattr(self, f)) for f in MOL_DEDUP_TOTALS}


class _MolCollapseTotals(C.Structure):
    """td_mol_collapse_totals (include/tagdust_molecules.h)"""
    _fields_ = [(f, C.c_int64) for f in MOL_COLLAPSE_TOTALS]

    def as_dict(self):
        return {f: int(getattr(self, f)) for f in MOL_COLLAPSE_TOTALS}


class _MolMate(C.Structure):
    """td_mol_mate (include/tagdust_molecules.h)"""
    _fields_ = [("codes", C.c_void_p), ("offs", C.c_void_p), ("bases", C.c_int32)]


class _RunReport(C.Structure):
    """td_run_report (include/tagdust_run.h)"""
    _fields_ = [("error", C.c_char * 1024), ("counts", C.c_int64 * NUM_COUNTERS), ("n_artifacts", C.c_int32),
                ("artifact_hits", C.POINTER(C.c_int64)), ("artifact_names", C.POINTER(C.c_char_p)), ("n_files", C.c_int32),
                ("thresholds", C.c_float * 8), ("selected_threshold", C.c_float), ("architectures", C.c_char_p * 8),
                ("stream", _StreamStats), ("arch_s", C.c_double), ("stats_s", C.c_double), ("calibration_s", C.c_double),
                ("compile_wait_s", C.c_double), ("stream_s", C.c_double), ("stats_on_device", C.c_int32), ("log", C.c_char_p),
                ("n_unknown", C.c_int64), ("unknown", C.c_void_p), ("unknown_totals", _CensusTotals),
                ("molecules", C.c_void_p), ("molecules_totals", _MolTotals), ("dedup", C.c_int32), ("dedup_totals", _MolDedupTotals),
                ("collapse", C.c_int32), ("collapse_totals", _MolCollapseTotals), ("molecules_collapsed", C.c_void_p),
                ("dedup_collapsed", C.c_int32), ("survey_s", C.c_double)]


class _RunReportSamples(C.Structure):
    """td_run_report as it is now: _RunReport -- whose last fields tests/test_dedup_collapsed.py pins -- and the fields appended
    behind them; this is the structure td_run_execute fills"""
    _fields_ = _RunReport._fields_ + [("n_samples", C.c_int32), ("n_sample_keys", C.c_int64), ("samples", C.c_void_p),
                                      ("samples_totals", _SamplesTotals)]


class _RunReportQuality(C.Structure):
    """td_run_report as it is now: _RunReportSamples and the fields appended behind it; this is the structure td_run_execute fills"""
    _fields_ = _RunReportSamples._fields_ + [("quality", C.c_int32), ("quality_totals", _QualTotals)]


class _RunOptsJoin(C.Structure):
    """td_run_opts as it is now: _RunOptsQuality and the field appended behind it"""
    _fields_ = _RunOptsQuality._fields_ + [("join_barcodes", C.c_int32)]


class _RunReportJoin(C.Structure):
    """td_run_report as it is now: _RunReportQuality and the field appended behind it; this is the structure td_run_execute fills"""
    _fields_ = _RunReportQuality._fields_ + [("partner_failed", C.c_int64)]


def _run_lib():
    lib = load_library()
    lib.td_run_parse_args.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.POINTER(_RunOptsJoin)), C.c_char_p, C.c_size_t]
    lib.td_run_opts_free.argtypes = [C.POINTER(_RunOptsJoin)]
    lib.td_run_opts_free.restype = None
    lib.td_run_last_error.restype = C.c_char_p
    lib.td_run_plan.argtypes = [C.POINTER(_RunOptsJoin), C.POINTER(C.c_void_p)]
    lib.td_run_plan_free.argtypes = [C.c_void_p]
    lib.td_run_plan_free.restype = None
    lib.td_run_plan_describe.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    lib.td_run_plan_describe.restype = C.c_int64
    lib.td_run_output_files_describe.argtypes = [C.POINTER(_RunOptsJoin), C.POINTER(C.c_char_p), C.c_int32, C.c_char_p, C.c_int64]
    lib.td_run_output_files_describe.restype = C.c_int64
    lib.td_run_arch_file_describe.argtypes = [C.c_char_p, C.c_char_p, C.c_int64]
    lib.td_run_arch_file_describe.restype = C.c_int64
    lib.td_run_execute.argtypes = [C.POINTER(_RunOptsJoin), C.POINTER(_RunReportJoin)]
    lib.td_run_report_clear.argtypes = [C.POINTER(_RunReportJoin)]
    lib.td_run_report_clear.restype = None
    # (the summary reads the report's leading fields alone -- counts, threshold, artifacts: a _RunReport will do as well)
    lib.td_run_format_summary.argtypes = [C.POINTER(_RunOptsJoin), C.c_void_p, C.c_char_p, C.c_int64]
    lib.td_run_format_summary.restype = C.c_int64
    return lib


class RunOpts:
    """td_run_parse_args: the tagdust command line (without the program name) as td_run_opts; .o is the C structure."""

    def __init__(self, args):
        self.lib = _run_lib()
        argv = [b"tagdust-hip"] + [os.fsencode(a) for a in args]
        arr = (C.c_char_p * len(argv))(*argv)
        self.p = C.POINTER(_RunOptsJoin)()
        err = C.create_string_buffer(1024)
        if self.lib.td_run_parse_args(len(argv), arr, C.byref(self.p), err, len(err)) != 0:
            self.p = None
            raise TdError(err.value.decode())
        self.o = self.p.contents

    def close(self):
        if getattr(self, "p", None):
            self.lib.td_run_opts_free(self.p)
            self.p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _text_of(call):
    n = int(call(None, 0))
    if n < 0:
        raise TdError(_run_lib().td_run_last_error().decode())
    buf = C.create_string_buffer(n + 1)
    call(buf, n + 1)
    return buf.value.decode()


def run_plan(args):
    """td_run_plan + td_run_plan_describe: the decisions of a run that need no data (no GPU), one "key: value" line each."""
    o = RunOpts(args)
    try:
        plan = C.c_void_p()
        if o.lib.td_run_plan(o.p, C.byref(plan)) != 0:
            raise TdError(o.lib.td_run_last_error().decode())
        try:
            return _text_of(lambda b, n: o.lib.td_run_plan_describe(plan, b, n))
        finally:
            o.lib.td_run_plan_free(plan)
    finally:
        o.close()


def run_output_files(args, architectures):
    """td_run_output_files_describe: the output files of a run with these per-file architectures ("-1 B:ACGT -2 R:N" each)."""
    o = RunOpts(args)
    try:
        arr = (C.c_char_p * len(architectures))(*[a.encode() for a in architectures])
        return _text_of(lambda b, n: o.lib.td_run_output_files_describe(o.p, arr, len(architectures), b, n)).splitlines()
    finally:
        o.close()


def run_arch_file(path):
    """td_run_arch_file_describe: the candidate architectures of an -arch file, one list of "-k segment" words per candidate."""
    lib = _run_lib()
    return _text_of(lambda b, n: lib.td_run_arch_file_describe(os.fsencode(path), b, n)).splitlines()


def run_execute(args):
    """td_run_execute: a whole run from the tagdust command line (without the program name); returns the report as a dict."""
    o = RunOpts(args)
    rep = _RunReportJoin()
    try:
        rc = o.lib.td_run_execute(o.p, C.byref(rep))
        if rc != 0:
            raise TdError(rep.error.decode())
        n, k = int(rep.n_artifacts), int(rep.n_files)
        return {
            "counts": np.array(list(rep.counts), np.int64),
            "artifact_hits": {rep.artifact_names[j].decode(): int(rep.artifact_hits[j]) for j in range(n)},
            "thresholds": [float(rep.thresholds[i]) for i in range(k)],
            "architectures": [rep.architectures[i].decode() for i in range(k)],
            "stream": {f: getattr(rep.stream, f) for f, _ in _StreamStats._fields_},
            "seconds": {f: getattr(rep, f + "_s") for f in ("arch", "stats", "calibration", "compile_wait", "stream")},
            "stats_on_device": bool(rep.stats_on_device), "log": (rep.log or b"").decode(),
            "unknown": _census_entries(rep.unknown, int(rep.n_unknown)), "unknown_totals": rep.unknown_totals.as_dict(),
            "molecules": _mol_rows(rep.molecules) if rep.molecules else None, "molecules_totals": rep.molecules_totals.as_dict(),
            "dedup_totals": rep.dedup_totals.as_dict() if rep.dedup else None,
            "collapse_totals": rep.collapse_totals.as_dict() if rep.collapse else None,
            "molecules_collapsed": _mol_rows(rep.molecules_collapsed) if rep.molecules_collapsed else None,
            "dedup_collapsed": bool(rep.dedup_collapsed), "survey_s": float(rep.survey_s),
            "samples": _census_entries(rep.samples, int(rep.n_sample_keys)) if rep.n_samples else None,
            "samples_totals": rep.samples_totals.as_dict() if rep.n_samples else None,
            "quality_totals": rep.quality_totals.as_dict() if rep.quality else None,
            "partner_failed": int(rep.partner_failed),
        }
    finally:
        o.lib.td_run_report_clear(C.byref(rep))
        o.close()


def _census_entries(ptr, n):
    """n td_census_entry at ptr, copied"""
    out = np.zeros(n, CENSUS_ENTRY_DTYPE)
    if n:
        C.memmove(out.ctypes.data, ptr, n * CENSUS_ENTRY_DTYPE.itemsize)
    return out


def _census_lib():
    lib = load_library()
    lib.td_census_enable.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.c_int32]
    lib.td_census_disable.argtypes = [C.c_void_p]
    lib.td_census_reset.argtypes = [C.c_void_p]
    lib.td_census_get.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(_CensusTotals)]
    lib.td_census_host.argtypes = [C.POINTER(_ModelDesc), C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                   C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(_CensusTotals)]
    lib.td_census_merge.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    lib.td_census_key_text.argtypes = [C.c_uint64, C.c_char_p]
    lib.td_census_free.argtypes = [C.c_void_p]
    lib.td_census_free.restype = None
    return lib


def census_host(md, seq, offs, read_type, labels, segment=-1, mask=CENSUS_DEFAULT_MASK):
    """td_census_host: the census of a batch from host arrays (no GPU).  md: model mapping; read_type: the reads' final outcomes
    (td_batch_download's, or the oracle's); labels as td_batch_download leaves them.  Returns (entries, totals dict)."""
    lib = _census_lib()
    desc, keep = make_model_desc(md)
    seq = np.ascontiguousarray(seq, np.uint8)
    offs = np.ascontiguousarray(offs, np.int64)
    labels = np.ascontiguousarray(labels, np.int8)
    rr = np.zeros(len(offs) - 1, RESULT_DTYPE)
    rr["read_type"] = np.asarray(read_type)
    ptr, n, tot = C.c_void_p(), C.c_int64(), _CensusTotals()
    rc = lib.td_census_host(C.byref(desc), int(segment), int(mask), seq.ctypes.data, offs.ctypes.data, len(offs) - 1, rr.ctypes.data,
                            labels.ctypes.data, C.byref(ptr), C.byref(n), C.byref(tot))
    del keep
    if rc != 0:
        raise TdError(lib.td_last_error(None).decode())
    try:
        return _census_entries(ptr, n.value), tot.as_dict()
    finally:
        lib.td_census_free(ptr)


def census_merge(a, b):
    """td_census_merge: the sum of two census results, in td_census_get's order."""
    lib = _census_lib()
    a = np.ascontiguousarray(a, CENSUS_ENTRY_DTYPE)
    b = np.ascontiguousarray(b, CENSUS_ENTRY_DTYPE)
    ptr, n = C.c_void_p(), C.c_int64()
    if lib.td_census_merge(a.ctypes.data, len(a), b.ctypes.data, len(b), C.byref(ptr), C.byref(n)) != 0:
        raise TdError(lib.td_last_error(None).decode())
    try:
        return _census_entries(ptr, n.value)
    finally:
        lib.td_census_free(ptr)


def census_key_text(key):
    """td_census_key_text: the bases a key spells ("ACGTTG")."""
    lib = _census_lib()
    buf = C.create_string_buffer(32)
    if lib.td_census_key_text(int(key), buf) != 0:
        raise TdError(lib.td_last_error(None).decode())
    return buf.value.decode()


def census_key(word):
    """the key of a word of 1..28 bases over ACGT (tagdust_census.h)"""
    assert 1 <= len(word) <= CENSUS_MAX_WORD
    v = 0
    for ch in word:
        v = (v << 2) | "ACGT".index(ch)
    return (len(word) << 56) | v


def _samples_lib():
    lib = _census_lib()
    lib.td_samples_enable.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p), C.c_int32, C.c_int32]
    lib.td_samples_disable.argtypes = [C.c_void_p]
    lib.td_samples_reset.argtypes = [C.c_void_p]
    lib.td_samples_get.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(_SamplesTotals)]
    lib.td_samples_name.argtypes = [C.c_void_p, C.c_int32]
    lib.td_samples_name.restype = C.c_char_p
    lib.td_samples_key.argtypes = [C.c_void_p, C.c_int32]
    lib.td_samples_key.restype = C.c_uint64
    lib.td_samples_key_calls.argtypes = [C.c_uint64, C.c_void_p, C.POINTER(C.c_int32)]
    lib.td_samples_host.argtypes = [C.POINTER(_ModelDesc), C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                    C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(_SamplesTotals)]
    lib.td_samples_export_enable.argtypes = [C.c_void_p, C.c_int32]
    lib.td_samples_export_disable.argtypes = [C.c_void_p]
    lib.td_samples_export_next.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.td_samples_join_enable.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    lib.td_samples_join_next.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.td_samples_join_get.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(_SamplesJoinTotals)]
    lib.td_samples_export_host.argtypes = [C.POINTER(_ModelDesc), C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.td_samples_join_host.argtypes = [C.POINTER(_ModelDesc), C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                         C.POINTER(_SamplesJoinTotals)]
    return lib


def _samples_sheet(tuples):
    """a sheet as the int32 [n_samples, m] array the library reads"""
    t = np.ascontiguousarray(tuples, np.int32)
    if t.ndim == 1:
        t = t.reshape(-1, 1)
    return t


def samples_host(md, tuples, offs, res, labels):
    """td_samples_host: sample assignment of a batch from host arrays (no GPU).  md: model mapping; tuples: the sheet, one row of m
    HMM indices per sample; res: RESULT_DTYPE records (td_batch_download's, or the oracle's), left alone; labels as
    td_batch_download leaves them.  Returns (the rewritten records, entries, totals dict)."""
    lib = _samples_lib()
    desc, keep = make_model_desc(md)
    t = _samples_sheet(tuples)
    offs = np.ascontiguousarray(offs, np.int64)
    labels = np.ascontiguousarray(labels, np.int8)
    rr = np.array(res, RESULT_DTYPE, copy=True)
    ptr, n, tot = C.c_void_p(), C.c_int64(), _SamplesTotals()
    rc = lib.td_samples_host(C.byref(desc), t.ctypes.data, len(t), offs.ctypes.data, len(offs) - 1, rr.ctypes.data, labels.ctypes.data,
                             C.byref(ptr), C.byref(n), C.byref(tot))
    del keep
    if rc != 0:
        raise TdError(lib.td_last_error(None).decode())
    try:
        return rr, _census_entries(ptr, n.value), tot.as_dict()
    finally:
        lib.td_census_free(ptr)


def samples_export_host(md, first_column, offs, res, labels):
    """td_samples_export_host: the export words (uint32, one per read) of a batch from host arrays (no GPU); the model's own 'B'
    segments are columns first_column.. of the join"""
    lib = _samples_lib()
    desc, keep = make_model_desc(md)
    offs = np.ascontiguousarray(offs, np.int64)
    labels = np.ascontiguousarray(labels, np.int8)
    rr = np.ascontiguousarray(np.array(res, RESULT_DTYPE, copy=True))
    words = np.zeros(max(len(offs) - 1, 1), np.uint32)
    rc = lib.td_samples_export_host(C.byref(desc), int(first_column), offs.ctypes.data, len(offs) - 1, rr.ctypes.data, labels.ctypes.data,
                                    words.ctypes.data)
    del keep
    if rc != 0:
        raise TdError(lib.td_last_error(None).decode())
    return words[:len(offs) - 1]


def samples_join_host(md, tuples, first_column, column_hmms, words, offs, res, labels):
    """td_samples_join_host: the join of a primary's batch with its partners' export words from host arrays (no GPU).  tuples: the
    sheet, one row of len(column_hmms) HMM indices per sample.  Returns (the rewritten records, entries, totals dict with
    partner_failed)."""
    lib = _samples_lib()
    desc, keep = make_model_desc(md)
    t = _samples_sheet(tuples)
    hm = np.ascontiguousarray(column_hmms, np.int32)
    offs = np.ascontiguousarray(offs, np.int64)
    labels = np.ascontiguousarray(labels, np.int8)
    w = np.ascontiguousarray(words, np.uint32)
    assert len(w) == len(offs) - 1
    if len(w) == 0:
        w = np.zeros(1, np.uint32)
    rr = np.array(res, RESULT_DTYPE, copy=True)
    ptr, n, tot = C.c_void_p(), C.c_int64(), _SamplesJoinTotals()
    rc = lib.td_samples_join_host(C.byref(desc), t.ctypes.data, len(t), len(hm), int(first_column), hm.ctypes.data, w.ctypes.data,
                                  offs.ctypes.data, len(offs) - 1, rr.ctypes.data, labels.ctypes.data, C.byref(ptr), C.byref(n), C.byref(tot))
    del keep
    if rc != 0:
        raise TdError(lib.td_last_error(None).decode())
    try:
        return rr, _census_entries(ptr, n.value), tot.as_dict()
    finally:
        lib.td_census_free(ptr)


def samples_key(calls):
    """td_samples_key: the key of a read's calls, one per chosen segment (-1: none)"""
    c = np.ascontiguousarray(calls, np.int32)
    key = int(_samples_lib().td_samples_key(c.ctypes.data, len(c)))
    if key == 0:
        raise TdError("td_samples_key: %r are no calls" % (list(calls),))
    return key


def samples_key_calls(key):
    """td_samples_key_calls: the calls a key stands for, one per chosen segment (-1: none)"""
    lib = _samples_lib()
    calls, m = np.zeros(SAMPLES_MAX_SEGMENTS, np.int32), C.c_int32()
    if lib.td_samples_key_calls(int(key), calls.ctypes.data, C.byref(m)) != 0:
        raise TdError(lib.td_last_error(None).decode())
    return [int(c) for c in calls[:m.value]]


def _qual_lib():
    lib = load_library()
    lib.td_qual_pack.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
    lib.td_qual_host.argtypes = [C.POINTER(_ModelDesc), C.POINTER(_QualParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.POINTER(_QualTotals)]
    lib.td_qual_enable.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.td_qual_disable.argtypes = [C.c_void_p]
    lib.td_qual_reset.argtypes = [C.c_void_p]
    lib.td_qual_get.argtypes = [C.c_void_p, C.POINTER(_QualTotals)]
    lib.td_qual_next.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    return lib


def qual_pack(qual, thr):
    """td_qual_pack: one low flag per quality byte, uint32 [(n + 31) // 32 + 1] with the spare zero word"""
    lib = _qual_lib()
    q = np.ascontiguousarray(qual, np.uint8)
    words = np.full((len(q) + 31) // 32 + 1, 0xFFFFFFFF, np.uint32)   # (every word is the call's to write)
    if lib.td_qual_pack(q.ctypes.data if len(q) else None, len(q), int(thr), words.ctypes.data) != 0:
        raise TdError(lib.td_last_error(None).decode())
    return words


def qual_host(md, offs, res, labels, qual, min_quality, offset=33, max_low=0, segments=QUAL_SEG_B | QUAL_SEG_F):
    """td_qual_host: the base-quality filter of a batch from host arrays (no GPU).  md: model mapping; res: RESULT_DTYPE records
    (td_batch_download's, or the oracle's), left alone; labels as td_batch_download leaves them; qual: read i's bytes at offs[i].
    Returns (the rewritten records, totals dict)."""
    lib = _qual_lib()
    desc, keep = make_model_desc(md)
    offs = np.ascontiguousarray(offs, np.int64)
    labels = np.ascontiguousarray(labels, np.int8)
    qual = np.ascontiguousarray(qual, np.uint8)
    rr = np.array(res, RESULT_DTYPE, copy=True)
    p, tot = _QualParams(int(min_quality), int(offset), int(max_low), int(segments)), _QualTotals()
    rc = lib.td_qual_host(C.byref(desc), C.byref(p), offs.ctypes.data, len(offs) - 1, rr.ctypes.data, labels.ctypes.data, qual.ctypes.data,
                          C.byref(tot))
    del keep
    if rc != 0:
        raise TdError(lib.td_last_error(None).decode())
    return rr, tot.as_dict()


def _mol_rows(ptr):
    """the NUM_BARCODE_BINS td_mol_row at ptr, copied"""
    out = np.zeros(NUM_BARCODE_BINS, MOL_ROW_DTYPE)
    C.memmove(out.ctypes.data, ptr, out.nbytes)
    return out


def _mol_lib():
    lib = _census_lib()
    lib.td_mol_enable.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.td_mol_disable.argtypes = [C.c_void_p]
    lib.td_mol_reset.argtypes = [C.c_void_p]
    lib.td_mol_entries.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(_MolTotals)]
    lib.td_mol_get.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_MolTotals)]
    lib.td_mol_summarise.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    lib.td_mol_host.argtypes = [C.POINTER(_ModelDesc), C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(_MolTotals)]
    lib.td_mol_key.argtypes = [C.c_int32, C.c_int32, C.c_uint64, C.c_int32]
    lib.td_mol_key.restype = C.c_uint64
    lib.td_mol_key_bin.argtypes = [C.c_uint64]
    lib.td_mol_key_bin.restype = C.c_int32
    lib.td_mol_dedup_enable.argtypes = [C.c_void_p]
    lib.td_mol_dedup_disable.argtypes = [C.c_void_p]
    lib.td_mol_dedup_get.argtypes = [C.c_void_p, C.POINTER(_MolDedupTotals)]
    lib.td_mol_dedup_host.argtypes = [C.POINTER(_ModelDesc), C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.POINTER(_MolDedupTotals)]
    lib.td_mol_dedup_freeze.argtypes = [C.c_void_p, C.POINTER(_MolCollapseTotals)]
    lib.td_mol_dedup_collapsed_host.argtypes = [C.POINTER(_ModelDesc), C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.POINTER(_MolDedupTotals), C.POINTER(_MolCollapseTotals)]
    lib.td_mol_collapse_enable.argtypes = [C.c_void_p]
    lib.td_mol_collapse_disable.argtypes = [C.c_void_p]
    lib.td_mol_origins.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(_MolTotals)]
    lib.td_mol_collapse_get.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_MolCollapseTotals)]
    lib.td_mol_collapse_entries.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(_MolCollapseTotals)]
    lib.td_mol_host_origins.argtypes = [C.POINTER(_ModelDesc), C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(_MolTotals)]
    lib.td_mol_collapse_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_int64), C.POINTER(_MolCollapseTotals)]
    lib.td_mol_mate_enable.argtypes = [C.c_void_p, C.c_int32]
    lib.td_mol_mate_disable.argtypes = [C.c_void_p]
    lib.td_mol_mate_next.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.td_mol_mate_filter_enable.argtypes = [C.c_void_p]
    lib.td_mol_mate_filter_disable.argtypes = [C.c_void_p]
    lib.td_mol_mate_types.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    mate = C.POINTER(_MolMate)
    lib.td_mol_host_mated.argtypes = lib.td_mol_host.argtypes[:7] + [mate] + lib.td_mol_host.argtypes[7:]
    lib.td_mol_host_origins_mated.argtypes = lib.td_mol_host_origins.argtypes[:7] + [mate] + lib.td_mol_host_origins.argtypes[7:]
    lib.td_mol_dedup_host_mated.argtypes = lib.td_mol_dedup_host.argtypes[:7] + [mate] + lib.td_mol_dedup_host.argtypes[7:]
    lib.td_mol_dedup_collapsed_host_mated.argtypes = (lib.td_mol_dedup_collapsed_host.argtypes[:7] + [mate] +
                                                      lib.td_mol_dedup_collapsed_host.argtypes[7:])
    lib.free.argtypes = [C.c_void_p]
    lib.free.restype = None
    return lib


def _mol_origin_array(ptr, n):
    """n td_mol_origin at ptr, copied"""
    out = np.zeros(n, MOL_ORIGIN_DTYPE)
    if n:
        C.memmove(out.ctypes.data, ptr, n * MOL_ORIGIN_DTYPE.itemsize)
    return out


def mol_collapse_host(entries, origins):
    """td_mol_collapse_host: the collapse of (key, count) entries with their origins, repeated keys added first (no GPU).  Returns
    (the roots with their collapsed counts, their origins, totals dict)."""
    lib = _mol_lib()
    e = np.ascontiguousarray(entries, CENSUS_ENTRY_DTYPE)
    o = np.ascontiguousarray(origins, MOL_ORIGIN_DTYPE)
    if len(e) != len(o):
        raise ValueError("entries and origins differ in length")
    ptr, optr, n, tot = C.c_void_p(), C.c_void_p(), C.c_int64(), _MolCollapseTotals()
    if lib.td_mol_collapse_host(e.ctypes.data, o.ctypes.data, len(e), C.byref(ptr), C.byref(optr), C.byref(n), C.byref(tot)) != 0:
        raise TdError(lib.td_last_error(None).decode())
    try:
        return _census_entries(ptr, n.value), _mol_origin_array(optr, n.value), tot.as_dict()
    finally:
        lib.td_census_free(ptr)
        lib.free(optr)


def _mol_host_call(symbol, md, seq, offs, res, labels, mate, prefix_bases, out):
    """What the eight host yardsticks over a batch share.  Prepares the model description, the arrays as the C side reads them and the
    td_mol_mate (mate: None, or (codes, offs, bases) with one mate per read in the reads' order); calls `symbol`, a *_mated entry point
    -- with mate None it is the unmated one, messages included --; raises TdError on failure; converts and frees what C allocated.
    out: "entries" (entries, totals), "origins" (entries, origins, totals), "marks" (is_duplicate, dedup totals) or "collapsed"
    (is_duplicate, dedup totals, collapse totals)."""
    lib = _mol_lib()
    desc, keep = make_model_desc(md)
    seq = np.ascontiguousarray(seq, np.uint8)
    if len(seq) == 0:
        seq = np.zeros(1, np.uint8)
    offs = np.ascontiguousarray(offs, np.int64)
    labels = np.ascontiguousarray(labels, np.int8)
    n = len(offs) - 1
    rr = np.zeros(n, RESULT_DTYPE)
    for f in ("read_type", "barcode", "fingerprint"):
        rr[f] = np.asarray(res[f])
    mp = None
    if mate is not None:
        mc = np.ascontiguousarray(mate[0], np.uint8)
        if len(mc) == 0:
            mc = np.zeros(1, np.uint8)
        mo = np.ascontiguousarray(mate[1], np.int64)
        if len(mo) != len(offs):
            raise ValueError("the mate batch has %d reads, the batch %d" % (len(mo) - 1, n))
        mm = _MolMate(mc.ctypes.data, mo.ctypes.data, int(mate[2]))
        mp = C.byref(mm)
    ptr, optr, count = C.c_void_p(), C.c_void_p(), C.c_int64()
    dup = np.zeros(max(n, 1), np.uint8)
    if out in ("entries", "origins"):
        tots = [_MolTotals()]
        outs = [C.byref(ptr)] + ([C.byref(optr)] if out == "origins" else []) + [C.byref(count)]
    else:
        tots = [_MolDedupTotals()] + ([_MolCollapseTotals()] if out == "collapsed" else [])
        outs = [dup.ctypes.data]
    rc = getattr(lib, symbol)(C.byref(desc), int(prefix_bases), seq.ctypes.data, offs.ctypes.data, n, rr.ctypes.data, labels.ctypes.data, mp,
                              *outs, *[C.byref(t) for t in tots])
    del keep
    if rc != 0:
        raise TdError(lib.td_last_error(None).decode())
    try:
        if out == "entries":
            return _census_entries(ptr, count.value), tots[0].as_dict()
        if out == "origins":
            return _census_entries(ptr, count.value), _mol_origin_array(optr, count.value), tots[0].as_dict()
        return (dup[:n].astype(bool),) + tuple(t.as_dict() for t in tots)
    finally:
        lib.td_census_free(ptr)
        lib.free(optr)


def mol_host_mated(md, seq, offs, res, labels, mate, prefix_bases=MOL_DEFAULT_PREFIX):
    """td_mol_host_mated: mol_host with the mate batch joined into the key (mate: (codes, offs, bases), or None for mol_host itself)."""
    return _mol_host_call("td_mol_host_mated", md, seq, offs, res, labels, mate, prefix_bases, "entries")


def mol_host_origins_mated(md, seq, offs, res, labels, mate, prefix_bases=MOL_DEFAULT_PREFIX):
    """td_mol_host_origins_mated: mol_host_origins with the mate batch joined into the key (mate as mol_host_mated takes it)."""
    return _mol_host_call("td_mol_host_origins_mated", md, seq, offs, res, labels, mate, prefix_bases, "origins")


def mol_dedup_host_mated(md, seq, offs, res, labels, mate, prefix_bases=MOL_DEFAULT_PREFIX):
    """td_mol_dedup_host_mated: mol_dedup_host with the mate batch joined into the key (mate as mol_host_mated takes it)."""
    return _mol_host_call("td_mol_dedup_host_mated", md, seq, offs, res, labels, mate, prefix_bases, "marks")


def mol_dedup_collapsed_host_mated(md, seq, offs, res, labels, mate, prefix_bases=MOL_DEFAULT_PREFIX):
    """td_mol_dedup_collapsed_host_mated: mol_dedup_collapsed_host with the mate batch joined into the key (mate as mol_host_mated
    takes it)."""
    return _mol_host_call("td_mol_dedup_collapsed_host_mated", md, seq, offs, res, labels, mate, prefix_bases, "collapsed")


def mol_host(md, seq, offs, res, labels, prefix_bases=MOL_DEFAULT_PREFIX):
    """td_mol_host: the molecule count of a batch from host arrays (no GPU).  md: model mapping; res: the reads' records
    (RESULT_DTYPE, or any mapping / structured array with read_type, barcode and fingerprint: td_batch_download's, or the
    oracle's); labels as td_batch_download leaves them.  Returns (entries, totals dict)."""
    return mol_host_mated(md, seq, offs, res, labels, None, prefix_bases)


def mol_host_origins(md, seq, offs, res, labels, prefix_bases=MOL_DEFAULT_PREFIX):
    """td_mol_host_origins: mol_host plus what every key was made of.  Returns (entries, origins MOL_ORIGIN_DTYPE, totals dict)."""
    return mol_host_origins_mated(md, seq, offs, res, labels, None, prefix_bases)


def mol_dedup_host(md, seq, offs, res, labels, prefix_bases=MOL_DEFAULT_PREFIX):
    """td_mol_dedup_host: which reads of a batch are not the first of their molecule, the reads in the given order (no GPU).
    Arguments as mol_host takes them.  Returns (is_duplicate, a bool per read; totals dict)."""
    return mol_dedup_host_mated(md, seq, offs, res, labels, None, prefix_bases)


def mol_dedup_collapsed_host(md, seq, offs, res, labels, prefix_bases=MOL_DEFAULT_PREFIX):
    """td_mol_dedup_collapsed_host: which reads are not the one read their collapsed molecule keeps -- the reads surveyed and the same
    reads replayed, in the given order (no GPU).  Arguments as mol_host takes them.  Returns (is_duplicate, a bool per read; dedup
    totals dict; collapse totals dict)."""
    return mol_dedup_collapsed_host_mated(md, seq, offs, res, labels, None, prefix_bases)


def mol_summarise(entries):
    """td_mol_summarise: one row per barcode bin (MOL_ROW_DTYPE[256]) from (key, count) entries."""
    lib = _mol_lib()
    e = np.ascontiguousarray(entries, CENSUS_ENTRY_DTYPE)
    rows = np.zeros(NUM_BARCODE_BINS, MOL_ROW_DTYPE)
    if lib.td_mol_summarise(e.ctypes.data, len(e), rows.ctypes.data) != 0:
        raise TdError(lib.td_last_error(None).decode())
    return rows


def mol_key(barcode, fingerprint, w, n):
    """td_mol_key: the key of a counted read"""
    return int(_mol_lib().td_mol_key(int(barcode), int(fingerprint), int(w), int(n)))


def mol_key_bin(key):
    return int(_mol_lib().td_mol_key_bin(int(key)))


def stream_release():
    """td_stream_release: free the page-locked batch buffers td_stream_run keeps for the next run of the process (at most 1 GiB;
    the library also frees them when the last context is destroyed)."""
    lib = load_library()
    lib.td_stream_release.restype = None
    lib.td_stream_release()


def spec_source(md):
    """The HIP source of the model-specialised kernel for this model (no GPU needed)."""
    lib = load_library()
    d, keep = make_model_desc(md)
    n = lib.td_spec_source(C.byref(d), None, 0)
    buf = C.create_string_buffer(int(n) + 1)
    lib.td_spec_source(C.byref(d), buf, int(n) + 1)
    return buf.value.decode()


PROBE_READS = 256


def spec_probe(md):
    """td_spec_probe: the reads a freshly loaded specialised kernel is checked with against the generic kernel, made from the
    model description alone (no GPU needed): (codes uint8 0..4, offs int64 [257])."""
    lib = load_library()
    lib.td_spec_probe.argtypes = [C.POINTER(_ModelDesc), C.c_void_p, C.c_int64, C.c_void_p]
    lib.td_spec_probe.restype = C.c_int64
    d, keep = make_model_desc(md)
    offs = np.zeros(PROBE_READS + 1, np.int64)
    n = int(lib.td_spec_probe(C.byref(d), None, 0, offs.ctypes.data))
    if n < 0:
        raise TdError("td_spec_probe: bad model description")
    codes = np.zeros(n, np.uint8)
    lib.td_spec_probe(C.byref(d), codes.ctypes.data, n, None)
    return codes, offs


def spec_probe_params():
    """The fixed parameters the probe is decoded with: dict(threshold, minlen, dust, window=(matchstart, matchend))."""
    lib = load_library()
    lib.td_spec_probe_params.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.td_spec_probe_params.restype = None
    t, ml, du, a, b = C.c_float(0), C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    lib.td_spec_probe_params(C.byref(t), C.byref(ml), C.byref(du), C.byref(a), C.byref(b))
    return dict(threshold=float(t.value), minlen=int(ml.value), dust=int(du.value), window=(int(a.value), int(b.value)))


def spec_prune_info(md, lcap):
    """Position-pruning tables of the specialised kernel for this model: dict with n_seg (leading segments pruned, 0 = none),
    sfx_first (first trailing segment pruned, S = none), z, and the tables fb, bwb, wa, wb, fbs, bws, wc, wd."""
    lib = load_library()
    d, keep = make_model_desc(md)
    tab = np.zeros(8 * (lcap + 8), np.float32)
    z, ns, sf = C.c_float(0), C.c_int32(0), C.c_int32(0)
    if lib.td_spec_prune_info(C.byref(d), int(lcap), tab.ctypes.data, C.byref(z), C.byref(ns), C.byref(sf)) != 0:
        raise RuntimeError("td_spec_prune_info failed")
    t = tab.reshape(8, lcap + 8)
    out = dict(n_seg=int(ns.value), sfx_first=int(sf.value), S=int(md["S"]), z=float(z.value))
    for k, name in enumerate(("fb", "bwb", "wa", "wb", "fbs", "bws", "wc", "wd")):
        out[name] = t[k]
    return out


def spec_restart_info(md, lcap):
    """Impulse-response tables of the restarted sweeps for this model: (gq [4, lcap + 8] leading segments, gf [4, lcap + 8]
    trailing segments, restart flag)."""
    lib = load_library()
    d, keep = make_model_desc(md)
    tab = np.zeros(8 * (lcap + 8), np.float32)
    r = C.c_int32(0)
    lib.td_spec_restart_info.argtypes = [C.POINTER(_ModelDesc), C.c_int32, C.c_void_p, C.POINTER(C.c_int32)]
    if lib.td_spec_restart_info(C.byref(d), int(lcap), tab.ctypes.data, C.byref(r)) != 0:
        raise RuntimeError("td_spec_restart_info failed")
    t = tab.reshape(8, lcap + 8)
    return t[:4], t[4:], int(r.value)


class TagdustHip:
    """One context per GPU (the analogue of run_pHMM's per-thread model copies)."""

    def __init__(self, device=0):
        self.lib = load_library()
        h = C.c_void_p()
        if self.lib.td_ctx_create(int(device), C.byref(h)) != 0:
            raise TdError(self.lib.td_last_error(None).decode())
        self.h = h
        self._keep = None
        self.offs = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.td_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise TdError(self.lib.td_last_error(self.h).decode())

    def set_option(self, name, value):
        self._chk(self.lib.td_set_option(self.h, name.encode(), int(value)))

    def set_artifacts(self, string=None, s_index=None, filter_error=2, n_threads=1):
        """-ref artifact filter (struct fasta's string / s_index); None switches it off."""
        if string is None:
            self._chk(self.lib.td_set_artifacts(self.h, None, None, 0, 0, 1))
            return
        a = np.ascontiguousarray(string, dtype=np.uint8)
        ix = np.ascontiguousarray(s_index, dtype=np.int32)
        self._chk(self.lib.td_set_artifacts(self.h, a.ctypes.data, ix.ctypes.data, len(ix) - 1, int(filter_error), int(n_threads)))

    def get_option(self, name):
        v = C.c_int32(0)
        self._chk(self.lib.td_get_option(self.h, name.encode(), C.byref(v)))
        return int(v.value)

    def upload_model(self, md):
        """md: mapping with S,H,C,avg_len,bg,n_hmm,n_col,skip,seg_type,seg_len,trans,eM,eI,sM,sI,label,A
        (the tables of struct model_bag; same keys as the golden fixtures)."""
        d, keep = make_model_desc(md)
        self._keep = keep
        self._chk(self.lib.td_model_upload(self.h, C.byref(d)))

    def spec_wait(self):
        """td_spec_wait: block until a background compile (option "async_compile") is finished and handed over."""
        self.lib.td_spec_wait.argtypes = [C.c_void_p]
        self._chk(self.lib.td_spec_wait(self.h))

    def set_params(self, threshold, minlen=16, dust=100):
        self._chk(self.lib.td_set_params(self.h, float(threshold), int(minlen), int(dust)))

    def set_window(self, matchstart=-1, matchend=-1):
        self._chk(self.lib.td_set_window(self.h, int(matchstart), int(matchend)))

    def set_batch_window(self, first_read=0, total_reads=0):
        """td_set_batch_window: the batches that follow are reads first_read.. of a batch of total_reads (0, 0: whole batches)"""
        self._chk(self.lib.td_set_batch_window(self.h, int(first_read), int(total_reads)))

    def upload_batch(self, codes, offs):
        codes = np.ascontiguousarray(codes, np.uint8)
        self.offs = np.ascontiguousarray(offs, np.int64)
        self._chk(self.lib.td_batch_upload(self.h, codes.ctypes.data, self.offs.ctypes.data, len(self.offs) - 1))

    def upload_batch_ascii(self, bases, offs):
        buf = np.frombuffer(bases, dtype=np.uint8) if isinstance(bases, (bytes, bytearray)) else np.ascontiguousarray(bases, np.uint8)
        self.offs = np.ascontiguousarray(offs, np.int64)
        self._chk(self.lib.td_batch_upload_ascii(self.h, buf.ctypes.data, self.offs.ctypes.data, len(self.offs) - 1))

    def run(self, mode=MODE_GET_LABEL):
        self._chk(self.lib.td_run(self.h, int(mode)))

    def sync(self):
        self._chk(self.lib.td_sync(self.h))

    def download(self, labels=True, seq=True):
        n = len(self.offs) - 1
        res = np.zeros(n, RESULT_DTYPE)
        lab = np.zeros(int(self.offs[-1]) + n, np.int8) if labels else None
        sq = np.zeros(int(self.offs[-1]), np.uint8) if seq else None
        self._chk(self.lib.td_batch_download(self.h, res.ctypes.data, lab.ctypes.data if labels else None,
                                             sq.ctypes.data if seq else None))
        return res, lab, sq

    def submit(self, bases, offs, mode=MODE_GET_LABEL, res=None, labels=None, seq_out=None, ascii=False):
        """td_submit: numpy arrays in (kept alive by the caller until wait()), result arrays named now; returns the ticket."""
        n = len(offs) - 1
        t = C.c_int64(0)
        self._chk(self.lib.td_submit(self.h, bases.ctypes.data, 1 if ascii else 0, offs.ctypes.data, n, int(mode),
                                     res.ctypes.data if res is not None else None,
                                     labels.ctypes.data if labels is not None else None,
                                     seq_out.ctypes.data if seq_out is not None else None, C.byref(t)))
        return int(t.value)

    def wait(self, ticket):
        self._chk(self.lib.td_wait(self.h, int(ticket)))

    def arch_scores(self, models, codes, offs):
        """td_arch_scores: backward score of every read under every candidate model, one launch; float32 [n_models, n]."""
        descs, keep = [], []
        for md in models:
            d, k = make_model_desc(md)
            descs.append(d)
            keep.append(k)
        ptrs = (C.c_void_p * len(descs))(*[C.addressof(d) for d in descs])
        codes = np.ascontiguousarray(codes, np.uint8)
        offs = np.ascontiguousarray(offs, np.int64)
        n = len(offs) - 1
        out = np.zeros((len(descs), n), np.float32)
        self._chk(self.lib.td_arch_scores(self.h, ptrs, len(descs), codes.ctypes.data, offs.ctypes.data, n, out.ctypes.data))
        return out

    def census_enable(self, segment=-1, mask=CENSUS_DEFAULT_MASK, log2_slots=20):
        self._chk(_census_lib().td_census_enable(self.h, int(segment), int(mask), int(log2_slots)))

    def census_disable(self):
        self._chk(_census_lib().td_census_disable(self.h))

    def census_reset(self):
        self._chk(_census_lib().td_census_reset(self.h))

    def census(self, cap=None):
        """td_census_get: (entries by count descending then key ascending -- at most cap of them --, totals dict)"""
        lib = _census_lib()
        n, tot = C.c_int64(), _CensusTotals()
        if cap is None:
            self._chk(lib.td_census_get(self.h, None, 0, C.byref(n), C.byref(tot)))
            cap = n.value
        out = np.zeros(int(cap), CENSUS_ENTRY_DTYPE)
        self._chk(lib.td_census_get(self.h, out.ctypes.data, int(cap), C.byref(n), C.byref(tot)))
        return out[:min(int(cap), n.value)], tot.as_dict()

    def samples_enable(self, tuples, names=None, log2_slots=16):
        """td_samples_enable: tuples = the sheet, one row of m HMM indices per sample; names = None, or one name (or None) per sample"""
        t = _samples_sheet(tuples)
        arr = None
        if names is not None:
            arr = (C.c_char_p * len(names))(*[None if s is None else s.encode() for s in names])
            assert len(names) == len(t)
        self._chk(_samples_lib().td_samples_enable(self.h, t.ctypes.data, arr, len(t), int(log2_slots)))

    def samples_disable(self):
        self._chk(_samples_lib().td_samples_disable(self.h))

    def samples_reset(self):
        self._chk(_samples_lib().td_samples_reset(self.h))

    def samples_name(self, s):
        name = _samples_lib().td_samples_name(self.h, int(s))
        return None if name is None else name.decode()

    def samples(self, cap=None):
        """td_samples_get: (entries by count descending then key ascending -- at most cap of them --, totals dict)"""
        lib = _samples_lib()
        n, tot = C.c_int64(), _SamplesTotals()
        if cap is None:
            self._chk(lib.td_samples_get(self.h, None, 0, C.byref(n), C.byref(tot)))
            cap = n.value
        out = np.zeros(int(cap), CENSUS_ENTRY_DTYPE)
        self._chk(lib.td_samples_get(self.h, out.ctypes.data, int(cap), C.byref(n), C.byref(tot)))
        return out[:min(int(cap), n.value)], tot.as_dict()

    def samples_export_enable(self, first_column=0):
        """td_samples_export_enable: from now on every MODE_GET_LABEL batch leaves its export words in the array samples_export_next named"""
        self._chk(_samples_lib().td_samples_export_enable(self.h, int(first_column)))

    def samples_export_disable(self):
        self._chk(_samples_lib().td_samples_export_disable(self.h))

    def samples_export_next(self, words, n_reads):
        """td_samples_export_next: the uint32 array (numpy or PinnedArray view, kept alive by the caller until the batch has been
        waited for; None: no array) that receives the next MODE_GET_LABEL batch's export words"""
        self._chk(_samples_lib().td_samples_export_next(self.h, words.ctypes.data if words is not None else None, int(n_reads)))

    def samples_join_enable(self, tuples, column_hmms, first_column=0, names=None, log2_slots=16):
        """td_samples_join_enable: the sheet has len(column_hmms) columns, this context's own 'B' segments are columns first_column.."""
        t = _samples_sheet(tuples)
        hm = np.ascontiguousarray(column_hmms, np.int32)
        arr = None
        if names is not None:
            arr = (C.c_char_p * len(names))(*[None if s is None else s.encode() for s in names])
            assert len(names) == len(t)
        self._chk(_samples_lib().td_samples_join_enable(self.h, t.ctypes.data, arr, len(t), int(log2_slots), len(hm), int(first_column),
                                                        hm.ctypes.data))

    def samples_join_next(self, words, n_reads):
        """td_samples_join_next: the partner words (uint32, one per read, the caller's order) of the next MODE_GET_LABEL batch; read
        when the batch is staged (upload_batch or submit has returned)"""
        self._chk(_samples_lib().td_samples_join_next(self.h, words.ctypes.data if words is not None else None, int(n_reads)))

    def samples_join(self, cap=None):
        """td_samples_join_get: (entries as samples(), totals dict with partner_failed)"""
        lib = _samples_lib()
        n, tot = C.c_int64(), _SamplesJoinTotals()
        if cap is None:
            self._chk(lib.td_samples_join_get(self.h, None, 0, C.byref(n), C.byref(tot)))
            cap = n.value
        out = np.zeros(int(cap), CENSUS_ENTRY_DTYPE)
        self._chk(lib.td_samples_join_get(self.h, out.ctypes.data, int(cap), C.byref(n), C.byref(tot)))
        return out[:min(int(cap), n.value)], tot.as_dict()

    def qual_enable(self, min_quality, offset=33, max_low=0, segments=QUAL_SEG_B | QUAL_SEG_F):
        """td_qual_enable: drop extracted reads with more than max_low barcode / UMI bases below min_quality"""
        self._chk(_qual_lib().td_qual_enable(self.h, int(min_quality), int(offset), int(max_low), int(segments)))

    def qual_disable(self):
        self._chk(_qual_lib().td_qual_disable(self.h))

    def qual_reset(self):
        self._chk(_qual_lib().td_qual_reset(self.h))

    def qual_next(self, qual, n_reads):
        """td_qual_next: the quality bytes of the next TD_MODE_GET_LABEL batch, read i's at qual[offs[i]:]; a numpy uint8 array the
        caller keeps alive until the batch is staged (upload_batch or submit has returned)"""
        self._chk(_qual_lib().td_qual_next(self.h, qual.ctypes.data if qual is not None else None, int(n_reads)))

    def qual_totals(self):
        """td_qual_get: the totals dict (waits for the queued work)"""
        tot = _QualTotals()
        self._chk(_qual_lib().td_qual_get(self.h, C.byref(tot)))
        return tot.as_dict()

    def mol_enable(self, prefix_bases=MOL_DEFAULT_PREFIX, log2_slots=16):
        self._chk(_mol_lib().td_mol_enable(self.h, int(prefix_bases), int(log2_slots)))

    def mol_disable(self):
        self._chk(_mol_lib().td_mol_disable(self.h))

    def mol_reset(self):
        self._chk(_mol_lib().td_mol_reset(self.h))

    def mol_mate_enable(self, mate_bases):
        """td_mol_mate_enable: from now on the first mate_bases bases of every read's mate belong to its key (an empty table)"""
        self._chk(_mol_lib().td_mol_mate_enable(self.h, int(mate_bases)))

    def mol_mate_disable(self):
        self._chk(_mol_lib().td_mol_mate_disable(self.h))

    def mol_mate_next(self, codes, offs):
        """td_mol_mate_next: the mate batch of the next batch staged for MODE_GET_LABEL (numpy uint8 / int64 arrays, or PinnedArray
        views; kept alive here until the next call, by the caller as long as the batch's own input)"""
        self._mate = (np.ascontiguousarray(codes, np.uint8) if len(codes) else np.zeros(1, np.uint8), np.ascontiguousarray(offs, np.int64))
        self._chk(_mol_lib().td_mol_mate_next(self.h, self._mate[0].ctypes.data, self._mate[1].ctypes.data, len(self._mate[1]) - 1))

    def mol_mate_filter_enable(self):
        """td_mol_mate_filter_enable: from now on every mate is judged as MODE_RNA_DUST judges (this context's dust, artifacts and
        thread ranges) and a read's outcome is the maximum of its own and its mate's (an empty table)"""
        self._chk(_mol_lib().td_mol_mate_filter_enable(self.h))

    def mol_mate_filter_disable(self):
        self._chk(_mol_lib().td_mol_mate_filter_disable(self.h))

    def mol_mate_types(self):
        """td_mol_mate_types: the mate types of the resident batch in the caller's order (int32)"""
        lib = _mol_lib()
        n = C.c_int64()
        self._chk(lib.td_mol_mate_types(self.h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.int32)
        self._chk(lib.td_mol_mate_types(self.h, out.ctypes.data, n.value, C.byref(n)))
        return out[:n.value]

    def mol_dedup_enable(self):
        """td_mol_dedup_enable: from now on a read that is not the first of its molecule gets read_type EXTRACT_DUPLICATE"""
        self._chk(_mol_lib().td_mol_dedup_enable(self.h))

    def mol_dedup_disable(self):
        self._chk(_mol_lib().td_mol_dedup_disable(self.h))

    def mol_dedup_get(self):
        """td_mol_dedup_get: {kept, duplicates, unjudged}"""
        tot = _MolDedupTotals()
        self._chk(_mol_lib().td_mol_dedup_get(self.h, C.byref(tot)))
        return tot.as_dict()

    def mol_dedup_freeze(self):
        """td_mol_dedup_freeze: the collapse, the keepers, and from now on every batch is replayed against them; collapse totals dict"""
        tot = _MolCollapseTotals()
        self._chk(_mol_lib().td_mol_dedup_freeze(self.h, C.byref(tot)))
        return tot.as_dict()

    def mol_collapse_enable(self):
        """td_mol_collapse_enable: from now on the table keeps what every key was made of"""
        self._chk(_mol_lib().td_mol_collapse_enable(self.h))

    def mol_collapse_disable(self):
        self._chk(_mol_lib().td_mol_collapse_disable(self.h))

    def _mol_with_origins(self, call, totals, cap):
        n = C.c_int64()
        if cap is None:
            self._chk(call(self.h, None, None, 0, C.byref(n), C.byref(totals)))
            cap = n.value
        e, o = np.zeros(max(int(cap), 1), CENSUS_ENTRY_DTYPE), np.zeros(max(int(cap), 1), MOL_ORIGIN_DTYPE)
        self._chk(call(self.h, e.ctypes.data, o.ctypes.data, int(cap), C.byref(n), C.byref(totals)))
        k = min(int(cap), n.value)
        return e[:k], o[:k], totals.as_dict()

    def mol_origins(self, cap=None):
        """td_mol_origins: (entries as mol_entries gives them, their origins MOL_ORIGIN_DTYPE, totals dict)"""
        return self._mol_with_origins(_mol_lib().td_mol_origins, _MolTotals(), cap)

    def mol_collapse_entries(self, cap=None):
        """td_mol_collapse_entries: (the roots with their collapsed counts, their origins, collapse totals dict)"""
        return self._mol_with_origins(_mol_lib().td_mol_collapse_entries, _MolCollapseTotals(), cap)

    def mol_collapse_get(self):
        """td_mol_collapse_get: (the summary from the collapsed counts, MOL_ROW_DTYPE[256], collapse totals dict)"""
        rows, tot = np.zeros(NUM_BARCODE_BINS, MOL_ROW_DTYPE), _MolCollapseTotals()
        self._chk(_mol_lib().td_mol_collapse_get(self.h, rows.ctypes.data, C.byref(tot)))
        return rows, tot.as_dict()

    def mol_entries(self, cap=None):
        """td_mol_entries: (the (key, count) pairs by count descending then key ascending -- at most cap of them --, totals dict)"""
        lib = _mol_lib()
        n, tot = C.c_int64(), _MolTotals()
        if cap is None:
            self._chk(lib.td_mol_entries(self.h, None, 0, C.byref(n), C.byref(tot)))
            cap = n.value
        out = np.zeros(int(cap), CENSUS_ENTRY_DTYPE)
        self._chk(lib.td_mol_entries(self.h, out.ctypes.data, int(cap), C.byref(n), C.byref(tot)))
        return out[:min(int(cap), n.value)], tot.as_dict()

    def mol_get(self):
        """td_mol_get: (the device's summary, MOL_ROW_DTYPE[256], totals dict)"""
        rows, tot = np.zeros(NUM_BARCODE_BINS, MOL_ROW_DTYPE), _MolTotals()
        self._chk(_mol_lib().td_mol_get(self.h, rows.ctypes.data, C.byref(tot)))
        return rows, tot.as_dict()

    def counts_reset(self):
        self._chk(self.lib.td_counts_reset(self.h))

    def counts(self):
        c = np.zeros(NUM_COUNTERS, np.int64)
        self._chk(self.lib.td_counts_get(self.h, c.ctypes.data))
        return c

    def artifact_hits(self, n_seq):
        """td_artifact_hits_get: reads per -ref sequence since the filter was set / the counters were reset; int64[n_seq]."""
        h = np.zeros(int(n_seq), np.int64)
        self._chk(self.lib.td_artifact_hits_get(self.h, h.ctypes.data, len(h)))
        return h

    def diag(self):
        """td_diag_get: the 64 diagnostic words of the development knobs (word k = historical slot 192 + k)."""
        d = np.zeros(NUM_DIAG_COUNTERS, np.int64)
        self._chk(self.lib.td_diag_get(self.h, d.ctypes.data))
        return d

    def last_kernel_ms(self):
        ms = C.c_float()
        self._chk(self.lib.td_last_kernel_ms(self.h, C.byref(ms)))
        return float(ms.value)

    def timeline_origin(self):
        self._chk(self.lib.td_timeline_origin(self.h))

    def last_kernel_times(self):
        """(start_ms, stop_ms, stream index) of the last batch's decode kernel, from the origin set by timeline_origin()."""
        a, b, k = C.c_float(), C.c_float(), C.c_int32()
        self._chk(self.lib.td_last_kernel_times(self.h, C.byref(a), C.byref(b), C.byref(k)))
        return float(a.value), float(b.value), int(k.value)

    def batch_info(self):
        n, w, s = C.c_int64(), C.c_int64(), C.c_int32()
        self._chk(self.lib.td_batch_info(self.h, C.byref(n), C.byref(w), C.byref(s)))
        return int(n.value), int(w.value), int(s.value)


class PinnedArray:
    """A numpy view of page-locked host memory from td_host_alloc (batch inputs / outputs the DMA engines use directly)."""

    def __init__(self, shape, dtype):
        self.lib = load_library()
        dt = np.dtype(dtype)
        n = int(np.prod(shape))
        self.ptr = self.lib.td_host_alloc(max(n * dt.itemsize, 1))
        if not self.ptr:
            raise TdError("td_host_alloc(%d bytes) failed" % (n * dt.itemsize))
        buf = (C.c_uint8 * (n * dt.itemsize)).from_address(self.ptr)
        self.array = np.frombuffer(buf, dtype=dt, count=n).reshape(shape)

    def free(self):
        if getattr(self, "ptr", None):
            self.array = None
            self.lib.td_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def bind_host_to_device(device):
    """td_bind_host_to_device: pin the calling thread to the CPUs of the NUMA node next to `device`; returns the node or -1."""
    return int(load_library().td_bind_host_to_device(int(device)))


def shard_bounds(n_reads, world, rank):
    """td_shard_bounds: run_pHMM's contiguous split (barcode_hmm.c:1911-1922); no GPU needed."""
    lib = load_library()
    lo, hi = C.c_int64(), C.c_int64()
    lib.td_shard_bounds(int(n_reads), int(world), int(rank), C.byref(lo), C.byref(hi))
    return int(lo.value), int(hi.value)


def count_outcomes(res, lens=None):
    """td_count_outcomes: the device counters restated on the host from per-read results; no GPU needed."""
    lib = load_library()
    res = np.ascontiguousarray(res, RESULT_DTYPE)
    c = np.zeros(NUM_COUNTERS, np.int64)
    ln = None if lens is None else np.ascontiguousarray(lens, np.int32)
    lib.td_count_outcomes(res.ctypes.data, ln.ctypes.data if ln is not None else None, len(res), c.ctypes.data)
    return c


class TagdustMulti:
    """Several GPUs driven from one process (include/tagdust_multi.h)."""

    def __init__(self, devices):
        self.lib = load_library()
        d = np.ascontiguousarray(devices, np.int32)
        h = C.c_void_p()
        if self.lib.td_multi_create(d.ctypes.data, len(d), C.byref(h)) != 0:
            raise TdError(self.lib.td_multi_last_error(None).decode())
        self.h = h
        self._keep = None

    def _chk(self, rc):
        if rc != 0:
            raise TdError(self.lib.td_multi_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.td_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload_model(self, md):
        d, keep = make_model_desc(md)
        self._keep = keep
        self._chk(self.lib.td_multi_model_upload(self.h, C.byref(d)))

    def set_params(self, threshold, minlen=16, dust=100):
        self._chk(self.lib.td_multi_set_params(self.h, float(threshold), int(minlen), int(dust)))

    def set_artifacts(self, string=None, s_index=None, filter_error=2, n_threads=1):
        if string is None:
            self._chk(self.lib.td_multi_set_artifacts(self.h, None, None, 0, 0, 1))
            return
        a = np.ascontiguousarray(string, np.uint8)
        ix = np.ascontiguousarray(s_index, np.int32)
        self._chk(self.lib.td_multi_set_artifacts(self.h, a.ctypes.data, ix.ctypes.data, len(ix) - 1, int(filter_error), int(n_threads)))

    def set_window(self, matchstart=-1, matchend=-1):
        self._chk(self.lib.td_multi_set_window(self.h, int(matchstart), int(matchend)))

    def decode(self, bases, offs, mode=MODE_GET_LABEL, labels=True, seq=True, ascii=False):
        bases = np.ascontiguousarray(bases, np.uint8)
        offs = np.ascontiguousarray(offs, np.int64)
        n = len(offs) - 1
        res = np.zeros(n, RESULT_DTYPE)
        lab = np.zeros(int(offs[-1]) + n, np.int8) if labels else None
        sq = np.zeros(int(offs[-1]), np.uint8) if seq else None
        self._chk(self.lib.td_multi_decode(self.h, bases.ctypes.data, 1 if ascii else 0, offs.ctypes.data, n, int(mode), res.ctypes.data,
                                           lab.ctypes.data if labels else None, sq.ctypes.data if seq else None))
        return res, lab, sq

    def counts(self):
        c = np.zeros(NUM_COUNTERS, np.int64)
        self._chk(self.lib.td_multi_counts(self.h, c.ctypes.data))
        return c

    def counts_reset(self):
        self._chk(self.lib.td_multi_counts_reset(self.h))

    def artifact_hits(self, n_seq):
        """td_multi_artifact_hits: reads per -ref sequence, summed over the devices; int64[n_seq]."""
        h = np.zeros(int(n_seq), np.int64)
        self._chk(self.lib.td_multi_artifact_hits(self.h, h.ctypes.data, len(h)))
        return h

    def uses_rccl(self):
        return bool(self.lib.td_multi_uses_rccl(self.h))


class _SimParams(C.Structure):
    _fields_ = [("seed", C.c_uint32), ("rng", C.c_int32), ("barnum", C.c_int32), ("barlen", C.c_int32), ("readlen", C.c_int32),
                ("readlen_mod", C.c_int32), ("numseq", C.c_int32), ("end_loss", C.c_int32), ("random_frac", C.c_float),
                ("error_rate", C.c_float), ("indel_frac", C.c_float), ("seq5", C.c_char_p), ("seq3", C.c_char_p)]


def simreads(barcodes, seed=42, rng=0, barnum=0, barlen=0, readlen=0, readlen_mod=0, numseq=0, end_loss=0, random_frac=0.0,
             error_rate=0.0, indel_frac=0.0, seq5=None, seq3=None):
    """td_simreads: the FASTQ text the reference's simreads writes for these options (bytes)."""
    lib = load_library()
    p = _SimParams(int(seed), int(rng), int(barnum), int(barlen), int(readlen), int(readlen_mod), int(numseq), int(end_loss),
                   float(random_frac), float(error_rate), float(indel_frac), seq5.encode() if seq5 else None, seq3.encode() if seq3 else None)
    arr = (C.c_char_p * max(len(barcodes), 1))(*[b.encode() for b in barcodes])
    out, n = C.c_void_p(), C.c_int64()
    lib.td_simreads.argtypes = [C.POINTER(_SimParams), C.POINTER(C.c_char_p), C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    lib.td_text_free.argtypes = [C.c_void_p]
    lib.td_text_free.restype = None
    if lib.td_simreads(C.byref(p), arr, len(barcodes), C.byref(out), C.byref(n)) != 0:
        raise TdError("td_simreads failed")
    try:
        return C.string_at(out, n.value)
    finally:
        lib.td_text_free(out)


# ---- include/tagdust_merge.h: merging of overlapping read pairs (used by the tests) ----
MERGE_ABI_SYMBOLS = ["td_merge_opts_default", "td_merge_last_error", "td_merge_tables_build", "td_merge_tables_free", "td_merge_host",
                     "td_merge_device", "td_merge_result_free", "td_merge_stream", "td_merge_parse_args", "td_merge_usage"]
MERGE_TABLE_AUTO, MERGE_TABLE_LDS, MERGE_TABLE_GLOBAL = 0, 1, 2
MERGE_WRITTEN, MERGE_BELOW, MERGE_NO_CANDIDATE = 0, 1, 2
MERGE_RECORD_DTYPE = np.dtype([("best_d", "<i4"), ("out_len", "<i4"), ("id", "<i4"), ("aligned", "<i4"), ("status", "<i4")])


class _MergeOpts(C.Structure):
    _fields_ = [("min_overlap", C.c_int32), ("threshold", C.c_float), ("n_threads", C.c_int32), ("batch_pairs", C.c_int32),
                ("device", C.c_int32), ("table_placement", C.c_int32)]


class _MergeTables(C.Structure):
    _fields_ = [("nq", C.c_int32), ("dim", C.c_int32), ("qchar", C.c_uint8 * 256), ("qindex", C.c_int16 * 256),
                ("profile", C.POINTER(C.c_float)), ("T", C.POINTER(C.c_float))]


class _MergeResult(C.Structure):
    _fields_ = [("n_pairs", C.c_int64), ("rec", C.c_void_p), ("out_off", C.POINTER(C.c_int64)), ("seq", C.c_void_p), ("qual", C.c_void_p),
                ("n_written", C.c_int64), ("n_below", C.c_int64), ("n_too_short", C.c_int64), ("table_in_lds", C.c_int32),
                ("n_on_host", C.c_int32), ("kernel_ms", C.c_float)]


class _MergeStats(C.Structure):
    _fields_ = [("n_pairs", C.c_int64), ("n_written", C.c_int64), ("n_below", C.c_int64), ("n_too_short", C.c_int64),
                ("n_batches", C.c_int64), ("bytes_in", C.c_int64), ("bytes_out", C.c_int64), ("wall_s", C.c_double), ("read_s", C.c_double),
                ("parse_s", C.c_double), ("tables_s", C.c_double), ("merge_s", C.c_double), ("kernel_s", C.c_double), ("write_s", C.c_double)]


def _merge_lib():
    lib = load_library()
    lib.td_merge_last_error.restype = C.c_char_p
    lib.td_merge_tables_build.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.POINTER(_MergeTables))]
    lib.td_merge_tables_free.argtypes = [C.POINTER(_MergeTables)]
    lib.td_merge_tables_free.restype = None
    for f in (lib.td_merge_host, lib.td_merge_device):
        f.argtypes = [C.POINTER(_Reads), C.POINTER(_Reads), C.POINTER(_MergeOpts), C.POINTER(C.POINTER(_MergeResult))]
    lib.td_merge_result_free.argtypes = [C.POINTER(_MergeResult)]
    lib.td_merge_result_free.restype = None
    lib.td_merge_stream.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(_MergeOpts), C.POINTER(_MergeStats)]
    return lib


def merge_tables(qual):
    """td_merge_tables_build for the quality characters in `qual` (bytes): nq, dim, qchar, qindex, profile [nq, 2], T [dim, dim]."""
    lib = _merge_lib()
    buf = np.frombuffer(bytes(qual), dtype=np.uint8)
    p = C.POINTER(_MergeTables)()
    if lib.td_merge_tables_build(buf.ctypes.data if len(buf) else None, len(buf), C.byref(p)) != 0:
        raise TdError(lib.td_merge_last_error().decode())
    try:
        t = p.contents
        nq, dim = int(t.nq), int(t.dim)
        return {"nq": nq, "dim": dim, "qchar": bytes(t.qchar[:nq]), "qindex": np.array(t.qindex[:], np.int16),
                "profile": np.ctypeslib.as_array(t.profile, shape=(nq, 2)).copy(), "T": np.ctypeslib.as_array(t.T, shape=(dim, dim)).copy()}
    finally:
        lib.td_merge_tables_free(p)


def merge_batch(reads1, reads2, device=None, min_overlap=16, threshold=0.0, n_threads=0, table_placement=MERGE_TABLE_AUTO):
    """td_merge_host (device None) or td_merge_device on two ParsedReads.  Returns rec (MERGE_RECORD_DTYPE), out_off, seq, qual (uint8
    arrays), the counts, table_in_lds, n_on_host, kernel_ms."""
    lib = _merge_lib()
    o = _MergeOpts(int(min_overlap), float(threshold), int(n_threads), 0, -1 if device is None else int(device), int(table_placement))
    p = C.POINTER(_MergeResult)()
    call = lib.td_merge_host if device is None else lib.td_merge_device
    if call(reads1._p, reads2._p, C.byref(o), C.byref(p)) != 0:
        raise TdError(lib.td_merge_last_error().decode())
    try:
        r = p.contents
        n = int(r.n_pairs)
        out_off = np.ctypeslib.as_array(r.out_off, shape=(n + 1,)).copy()
        total = int(out_off[-1])
        rec = np.frombuffer(C.string_at(r.rec, n * MERGE_RECORD_DTYPE.itemsize), dtype=MERGE_RECORD_DTYPE).copy()
        return {"rec": rec, "out_off": out_off, "seq": np.frombuffer(C.string_at(r.seq, total), np.uint8).copy(),
                "qual": np.frombuffer(C.string_at(r.qual, total), np.uint8).copy(), "n_written": int(r.n_written), "n_below": int(r.n_below),
                "n_too_short": int(r.n_too_short), "table_in_lds": int(r.table_in_lds), "n_on_host": int(r.n_on_host),
                "kernel_ms": float(r.kernel_ms)}
    finally:
        lib.td_merge_result_free(p)


def merge_text(res, names):
    """the records `merge` prints for a merge_batch result: "@<name of read 1>\\n<seq>\\n+\\n<qual>\\n" per written pair (bytes)"""
    seq, qual = res["seq"].tobytes(), res["qual"].tobytes()
    out = []
    for name, r, o in zip(names, res["rec"], res["out_off"]):
        n = int(r["out_len"])
        if n:
            out.append(b"@" + name + b"\n" + seq[o:o + n] + b"\n+\n" + qual[o:o + n] + b"\n")
    return b"".join(out)


def merge_stream(in1, in2, out_path, device=None, min_overlap=16, threshold=0.0, n_threads=0, batch_pairs=0):
    """td_merge_stream: two FASTQ files (plain, .gz, .bz2) to one file of merged reads; device None = the host path.  Returns the statistics."""
    lib = _merge_lib()
    o = _MergeOpts(int(min_overlap), float(threshold), int(n_threads), int(batch_pairs), -1 if device is None else int(device), MERGE_TABLE_AUTO)
    st = _MergeStats()
    if lib.td_merge_stream(os.fsencode(in1), os.fsencode(in2), os.fsencode(out_path), C.byref(o), C.byref(st)) != 0:
        raise TdError(lib.td_merge_last_error().decode())
    return {k: getattr(st, k) for k, _ in _MergeStats._fields_}
