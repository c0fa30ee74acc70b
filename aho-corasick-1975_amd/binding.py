"""ctypes bindings of libac75_amd.so (include/acm.h + include/acm_gpu.h)."""
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBNAME = "libac75_amd.so"

RECORD_DTYPE = np.dtype([("end_pos", "<u8"), ("length", "<u4"), ("keyword_id", "<u4")])

ACM_GPU_OK = 0
ACM_GPU_E_INELIGIBLE = -1
ACM_GPU_E_NODEVICE = -2
ACM_GPU_E_HIP = -3
ACM_GPU_E_OVERFLOW = -4
ACM_GPU_E_ARG = -5
ACM_GREP_MATCHING, ACM_GREP_INVERT = 0, 1
ACM_SPLIT_EVERY, ACM_SPLIT_RUNS = 0, 1
ACM_WORDS_LEFT, ACM_WORDS_RIGHT, ACM_WORDS_BOTH = 1, 2, 3
ACM_CONTEXT_SYMBOLS, ACM_CONTEXT_TEXTS, ACM_CONTEXT_EACH, ACM_CONTEXT_MERGE = 0, 1, 0, 2
ACM_CONTEXT_NONE = 0xFFFFFFFF
ACM_RULE_NO_MAX = 0xFFFFFFFF
ACM_SCORE_NO_CAP = 0xFFFFFFFF
ACM_SCORE_NONE = 0xFFFFFFFF
ACM_SCORE_TOP_MAX = 256
ACM_ANCHORED_PREFIXES, ACM_ANCHORED_LONGEST, ACM_ANCHORED_WHOLE = 1, 2, 3
ACM_LOOKUP_NONE = 0xFFFFFFFF
# the usual ASCII word set as inclusive (lo, hi) ranges: 0-9, A-Z, _, a-z (UTF-8 byte text adds (0x80, 0xFF))
ASCII_WORD = ((0x30, 0x39), (0x41, 0x5A), (0x5F, 0x5F), (0x61, 0x7A))


class ACMError(RuntimeError):
    def __init__(self, code, what):
        self.code = code
        msg = lib().acm_gpu_strerror(code).decode() if _lib is not None else str(code)
        super().__init__("%s: %s (code %d)" % (what, msg, code))


def library_path():
    # ACM_NATIVE_LIB lets tools/ load the diagnostic build (libac75_amd_diag.so) instead
    return os.environ.get("ACM_NATIVE_LIB") or os.path.join(_HERE, _LIBNAME)


def build_native(force=False):
    """Compile libac75_amd.so in-tree with the committed Makefile (hipcc --offload-arch=gfx950;
    cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    if force:
        subprocess.run(["make", "-s", "-C", csrc, "clean"], check=True)
    subprocess.run(["make", "-s", "-C", csrc], check=True)
    return library_path()


class MatchHolder(C.Structure):
    _fields_ = [("letters", C.POINTER(C.c_void_p)), ("length", C.c_size_t), ("value", C.c_void_p)]


class FlatInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("sym_bytes", "n_states", "n_keywords", "n_edges", "lmax", "max_outputs",
                                          "alpha_lo", "alpha_span", "width")]


class FlatView(C.Structure):
    _fields_ = [(n, C.POINTER(C.c_uint32)) for n in ("row_ptr", "edge_sym", "edge_next", "fail", "depth", "nb_outputs",
                                                     "term_kw", "out_link", "depth_start", "kw_state")] + [
        ("class_map", C.POINTER(C.c_uint16)), ("edge_letter", C.POINTER(C.c_uint32)), ("class_entries", C.c_uint32),
        ("n_classes", C.c_uint32), ("keys64", C.POINTER(C.c_uint64)), ("n_keys64", C.c_uint32),
        ("keys32", C.POINTER(C.c_uint32)), ("keys32_class", C.POINTER(C.c_uint32)), ("n_keys32", C.c_uint32),
        ("class_rep32", C.POINTER(C.c_uint32))]


class PlanInfo(C.Structure):
    _fields_ = [("device", C.c_int)] + [(n, C.c_uint32) for n in (
        "kernel", "entry_bytes", "width", "dense_rows", "lds_rows", "lds_hotfail", "lds_bytes", "block_threads", "grid_blocks",
        "chunk_bytes", "streams")] + [("table_bytes", C.c_uint64), ("delta_keywords", C.c_uint32), ("merges", C.c_uint32),
                                     ("records_direct", C.c_uint32), ("variant", C.c_uint32)]


class RulesInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("rules", "terms", "always_rules", "postings", "fast_texts", "wide_texts")]


class ScoreInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("classes", "terms", "postings", "always_classes", "fast_texts", "wide_texts")]


class PatternsInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("patterns", "terms", "anchor_keywords", "longest", "max_anchor_postings")]


class ChainsInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("chains", "terms", "max_terms", "max_gap", "max_postings", "max_last_postings")]


class ApproxInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("targets", "terms", "seed_keywords", "longest", "max_k", "max_postings")]


class NearInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("groups", "terms", "max_terms", "max_width", "max_postings")]


class TemplatesInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("templates", "terms", "classes", "seed_keywords", "longest", "max_k", "max_postings")]


class TemplateSpec(C.Structure):
    """ACMTemplateSpec: the arrays of a template set, host pointers"""
    _fields_ = [("spell_data", C.c_void_p), ("spell_off", C.c_void_p), ("cells", C.c_void_p), ("k", C.c_void_p), ("terms", C.c_void_p),
                ("tgt_ptr", C.c_void_p), ("n_templates", C.c_uint64), ("ranges", C.c_void_p), ("cls_ptr", C.c_void_p), ("cls_flags", C.c_void_p),
                ("n_classes", C.c_uint64)]


_lib = None

# every symbol include/acm.h and include/acm_gpu.h (with include/acm_segment.h, include/acm_score.h and include/acm_index.h) declare
EXPORTS = [
    "ACM_CMP_DEFAULT", "ACM_INCREMENTAL_STRING_MATCHING", "acm_create", "acm_initiate",
    "acm_insert_letter_of_keyword", "acm_insert_end_of_keyword", "acm_match", "acm_matcher_init", "acm_get_match",
    "acm_matcher_release", "acm_nb_keywords", "acm_foreach_keyword", "acm_release", "acm_print",
    "acm_gpu_strerror", "acm_gpu_device_count", "acm_get_keyword", "acm_flatten", "acm_flat_release", "acm_flat_info", "acm_flat_view",
    "acm_flat_dense_rows", "acm_flat_blob_bytes", "acm_flat_to_blob", "acm_flat_from_blob", "acm_flat_save",
    "acm_flat_load", "acm_flat_keyword", "acm_flatten_classes", "acm_gpu_plan_create_classes", "acm_gpu_plan_create", "acm_gpu_plan_create_flat", "acm_gpu_plan_update", "acm_gpu_plan_destroy",
    "acm_gpu_plan_info", "acm_gpu_scan_device", "acm_gpu_count_device", "acm_gpu_sort_tmp_bytes",
    "acm_gpu_sort_records_device", "acm_gpu_order_tmp_bytes", "acm_gpu_order_records_device", "acm_gpu_scan_ordered_tmp_bytes", "acm_gpu_scan_ordered_device", "acm_gpu_scan_host", "acm_scan", "acm_gpu_plan_timing",
    "acm_gpu_plan_timing_read", "acm_gpu_plan_timing_read_all", "acm_gpu_plan_status", "acm_gpu_synth_text",
    "acm_gpu_stream_open", "acm_gpu_stream_feed", "acm_gpu_stream_finish", "acm_gpu_stream_close",
    "acm_gpu_multi_create", "acm_gpu_multi_destroy", "acm_gpu_multi_shard_bounds", "acm_gpu_multi_scan_host",
    "acm_gpu_multi_scan_device", "acm_set_symbol_bytes", "acm_scan_path", "acm_gpu_wire_bits", "acm_gpu_pack_records_device",
    "acm_gpu_unpack_records_device", "acm_gpu_comm_unique_id", "acm_gpu_comm_init_rank", "acm_gpu_comm_free", "acm_gpu_comm_create",
    "acm_gpu_comm_destroy", "acm_gpu_comm_gather_records",
    "acm_gpu_scan_batch_tmp_bytes", "acm_gpu_scan_batch_device", "acm_gpu_scan_batch_host", "acm_scan_batch",
    "acm_gpu_flows_create", "acm_gpu_flows_destroy", "acm_gpu_flows_reset", "acm_gpu_scan_flows_tmp_bytes", "acm_gpu_scan_flows_device",
    "acm_gpu_scan_flows_host", "acm_scan_from",
    "acm_gpu_tally_tmp_bytes", "acm_gpu_tally_device", "acm_gpu_tally_form", "acm_gpu_tally_keywords", "acm_gpu_tally_host", "acm_tally",
    "acm_select_records", "acm_gpu_select_tmp_bytes", "acm_gpu_select_records_device", "acm_gpu_select_form",
    "acm_gpu_scan_select_tmp_bytes", "acm_gpu_scan_select_device", "acm_gpu_scan_select_host", "acm_select",
    "acm_replace_records", "acm_gpu_replace_tmp_bytes", "acm_gpu_replace_records_device", "acm_gpu_scan_replace_tmp_bytes",
    "acm_gpu_scan_replace_device", "acm_gpu_scan_replace_host", "acm_replace",
    "acm_tokens_records", "acm_gpu_tokens_tmp_bytes", "acm_gpu_tokens_records_device", "acm_gpu_scan_tokens_tmp_bytes",
    "acm_gpu_scan_tokens_device", "acm_gpu_scan_tokens_host", "acm_tokenize",
    "acm_grep_gather", "acm_gpu_grep_tmp_bytes", "acm_gpu_grep_device", "acm_gpu_grep_host", "acm_grep",
    "acm_split_offsets", "acm_gpu_split_tmp_bytes", "acm_gpu_split_device", "acm_gpu_split_host", "acm_gpu_grep_lines_host", "acm_grep_lines",
    "acm_tally_batch_records", "acm_gpu_tally_batch_tmp_bytes", "acm_gpu_tally_batch_device", "acm_gpu_tally_batch_host", "acm_tally_batch",
    "acm_words_records", "acm_gpu_words_tmp_bytes", "acm_gpu_words_records_device", "acm_gpu_scan_words_tmp_bytes", "acm_gpu_scan_words_device",
    "acm_gpu_scan_words_host", "acm_scan_words",
    "acm_context_records", "acm_gpu_context_tmp_bytes", "acm_gpu_context_records_device", "acm_gpu_scan_context_tmp_bytes",
    "acm_gpu_scan_context_device", "acm_gpu_scan_context_host", "acm_context",
    "acm_anchored_records", "acm_gpu_scan_anchored_tmp_bytes", "acm_gpu_scan_anchored_device", "acm_gpu_lookup_tmp_bytes", "acm_gpu_lookup_device",
    "acm_gpu_scan_anchored_host", "acm_gpu_lookup_host", "acm_scan_anchored", "acm_lookup",
    "acm_rules_check", "acm_rules_matrix", "acm_gpu_rules_create", "acm_gpu_rules_destroy", "acm_gpu_rules_info", "acm_gpu_rules_matrix_tmp_bytes",
    "acm_gpu_rules_matrix_device", "acm_gpu_rules_tmp_bytes", "acm_gpu_rules_device", "acm_gpu_rules_host", "acm_rules",
    "acm_patterns_check", "acm_patterns_records", "acm_gpu_patterns_create", "acm_gpu_patterns_destroy", "acm_gpu_patterns_info",
    "acm_gpu_patterns_tmp_bytes", "acm_gpu_patterns_records_device", "acm_gpu_scan_patterns_tmp_bytes", "acm_gpu_scan_patterns_device",
    "acm_gpu_scan_patterns_host", "acm_scan_patterns",
    "acm_approx_check", "acm_approx_split", "acm_approx_records", "acm_gpu_approx_create", "acm_gpu_approx_destroy", "acm_gpu_approx_info",
    "acm_gpu_approx_tmp_bytes", "acm_gpu_approx_records_device", "acm_gpu_scan_approx_tmp_bytes", "acm_gpu_scan_approx_device",
    "acm_gpu_scan_approx_host", "acm_scan_approx",
    "acm_templates_check", "acm_templates_split", "acm_templates_records", "acm_gpu_templates_create", "acm_gpu_templates_destroy",
    "acm_gpu_templates_info", "acm_gpu_templates_tmp_bytes", "acm_gpu_templates_records_device", "acm_gpu_scan_templates_tmp_bytes",
    "acm_gpu_scan_templates_device", "acm_gpu_scan_templates_host", "acm_scan_templates",
    "acm_edit_check", "acm_edit_records", "acm_gpu_edit_tmp_bytes", "acm_gpu_edit_records_device", "acm_gpu_scan_edit_tmp_bytes",
    "acm_gpu_scan_edit_device", "acm_gpu_scan_edit_host", "acm_scan_edit",
    "acm_chains_check", "acm_chains_records", "acm_gpu_chains_create", "acm_gpu_chains_destroy", "acm_gpu_chains_info",
    "acm_gpu_chains_tmp_bytes", "acm_gpu_chains_records_device", "acm_gpu_scan_chains_tmp_bytes", "acm_gpu_scan_chains_device",
    "acm_gpu_scan_chains_host", "acm_scan_chains",
    "acm_segment_records", "acm_gpu_segment_tmp_bytes", "acm_gpu_segment_records_device", "acm_gpu_scan_segment_tmp_bytes",
    "acm_gpu_scan_segment_device", "acm_gpu_scan_segment_host", "acm_segment",
    "acm_score_check", "acm_score_matrix", "acm_score_top", "acm_gpu_score_create", "acm_gpu_score_destroy", "acm_gpu_score_info",
    "acm_gpu_score_matrix_tmp_bytes", "acm_gpu_score_matrix_device", "acm_gpu_score_top_tmp_bytes", "acm_gpu_score_top_device",
    "acm_gpu_score_tmp_bytes", "acm_gpu_score_device", "acm_gpu_score_host", "acm_score",
    "acm_index_matrix", "acm_index_concat", "acm_gpu_index_matrix_tmp_bytes", "acm_gpu_index_matrix_device", "acm_gpu_index_concat_tmp_bytes",
    "acm_gpu_index_concat_device", "acm_gpu_index_tmp_bytes", "acm_gpu_index_device", "acm_gpu_index_host", "acm_index",
]

# every function include/acm_near.h declares (a list of its own: EXPORTS is the five headers above)
NEAR_EXPORTS = [
    "acm_near_check", "acm_near_records", "acm_gpu_near_create", "acm_gpu_near_destroy", "acm_gpu_near_info", "acm_gpu_near_tmp_bytes",
    "acm_gpu_near_records_device", "acm_gpu_scan_near_tmp_bytes", "acm_gpu_scan_near_device", "acm_gpu_scan_near_host", "acm_scan_near",
]

# every function include/acm_cooccur.h declares (a list of its own, as NEAR_EXPORTS is)
COOCCUR_EXPORTS = [
    "acm_cooccur_matrix", "acm_cooccur_add", "acm_gpu_cooccur_matrix_tmp_bytes", "acm_gpu_cooccur_matrix_device", "acm_gpu_cooccur_add_tmp_bytes",
    "acm_gpu_cooccur_add_device", "acm_gpu_cooccur_tmp_bytes", "acm_gpu_cooccur_device", "acm_gpu_cooccur_host", "acm_cooccur",
]
ACM_COOCCUR_PRODUCT, ACM_COOCCUR_DIAGONAL = 1, 2

# every function include/acm_chars.h declares (a list of its own, as NEAR_EXPORTS is)
CHARS_EXPORTS = [
    "acm_chars_positions", "acm_chars_records", "acm_gpu_chars_ruler_bytes", "acm_gpu_chars_ruler_tmp_bytes", "acm_gpu_chars_ruler_device",
    "acm_gpu_chars_tmp_bytes", "acm_gpu_chars_records_device", "acm_gpu_chars_positions_device", "acm_gpu_scan_chars_tmp_bytes",
    "acm_gpu_scan_chars_device", "acm_gpu_scan_chars_host", "acm_scan_chars",
]
ACM_CHARS_CODEPOINTS, ACM_CHARS_UTF16 = 1, 2
ACM_CHARS_EDGE_START, ACM_CHARS_EDGE_END, ACM_CHARS_EDGE_BAD = 1, 2, 4
# what Machine.scan_str returns: a match in the indices of the str itself
STR_MATCH_DTYPE = np.dtype([("start", "<u8"), ("stop", "<u8"), ("keyword_id", "<u4"), ("edge", "u1")])


def lib():
    """Loads the native library; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(or make -C aho-corasick-1975_amd/csrc) first" % path)
    L = C.CDLL(path)
    vp, sz, u64, u32, i32 = C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint32, C.c_int
    L.acm_create.restype = vp
    L.acm_create.argtypes = [vp, vp, vp]
    L.acm_initiate.restype = vp
    L.acm_initiate.argtypes = [vp]
    L.acm_insert_letter_of_keyword.restype = None
    L.acm_insert_letter_of_keyword.argtypes = [C.POINTER(vp), vp]
    L.acm_insert_end_of_keyword.restype = vp
    L.acm_insert_end_of_keyword.argtypes = [C.POINTER(vp), vp, vp]
    L.acm_match.restype = sz
    L.acm_match.argtypes = [C.POINTER(vp), vp]
    L.acm_matcher_init.restype = None
    L.acm_matcher_init.argtypes = [C.POINTER(MatchHolder)]
    L.acm_get_match.restype = None
    L.acm_get_match.argtypes = [vp, sz, C.POINTER(MatchHolder)]
    L.acm_matcher_release.restype = None
    L.acm_matcher_release.argtypes = [C.POINTER(MatchHolder)]
    L.acm_nb_keywords.restype = sz
    L.acm_nb_keywords.argtypes = [vp]
    L.acm_foreach_keyword.restype = None
    L.acm_foreach_keyword.argtypes = [vp, vp]
    L.acm_release.restype = None
    L.acm_release.argtypes = [vp]
    L.acm_print.restype = None
    L.acm_print.argtypes = [vp, vp, vp]
    L.acm_gpu_strerror.restype = C.c_char_p
    L.acm_gpu_strerror.argtypes = [i32]
    L.acm_gpu_device_count.restype = i32
    L.acm_gpu_device_count.argtypes = []
    L.acm_get_keyword.restype = i32
    L.acm_get_keyword.argtypes = [vp, u32, C.POINTER(MatchHolder)]
    L.acm_flatten.restype = i32
    L.acm_flatten.argtypes = [vp, C.POINTER(vp)]
    L.acm_flat_release.restype = None
    L.acm_flat_release.argtypes = [vp]
    L.acm_flat_info.restype = None
    L.acm_flat_info.argtypes = [vp, C.POINTER(FlatInfo)]
    L.acm_flat_view.restype = None
    L.acm_flat_view.argtypes = [vp, C.POINTER(FlatView)]
    L.acm_flat_dense_rows.restype = i32
    L.acm_flat_dense_rows.argtypes = [vp, u32, u32, vp]
    L.acm_flatten_classes.restype = i32
    L.acm_flatten_classes.argtypes = [vp, u32, C.POINTER(vp)]
    L.acm_gpu_plan_create_classes.restype = i32
    L.acm_gpu_plan_create_classes.argtypes = [vp, u32, i32, C.POINTER(vp)]
    L.acm_flat_blob_bytes.restype = sz
    L.acm_flat_blob_bytes.argtypes = [vp]
    L.acm_flat_to_blob.restype = i32
    L.acm_flat_to_blob.argtypes = [vp, vp, sz]
    L.acm_flat_from_blob.restype = i32
    L.acm_flat_from_blob.argtypes = [vp, sz, C.POINTER(vp)]
    L.acm_flat_save.restype = i32
    L.acm_flat_save.argtypes = [vp, C.c_char_p]
    L.acm_flat_load.restype = i32
    L.acm_flat_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.acm_flat_keyword.restype = i32
    L.acm_flat_keyword.argtypes = [vp, u32, vp, u32, C.POINTER(u32)]
    L.acm_gpu_plan_create.restype = i32
    L.acm_gpu_plan_create.argtypes = [vp, i32, C.POINTER(vp)]
    L.acm_gpu_plan_update.restype = i32
    L.acm_gpu_plan_update.argtypes = [vp, vp]
    L.acm_gpu_plan_create_flat.restype = i32
    L.acm_gpu_plan_create_flat.argtypes = [vp, i32, C.POINTER(vp)]
    L.acm_gpu_plan_destroy.restype = None
    L.acm_gpu_plan_destroy.argtypes = [vp]
    L.acm_gpu_plan_info.restype = None
    L.acm_gpu_plan_info.argtypes = [vp, C.POINTER(PlanInfo)]
    L.acm_gpu_scan_device.restype = i32
    L.acm_gpu_scan_device.argtypes = [vp, vp, u64, u64, u64, vp, u64, vp, vp]
    L.acm_gpu_count_device.restype = i32
    L.acm_gpu_count_device.argtypes = [vp, vp, u64, u64, vp, vp]
    L.acm_gpu_sort_tmp_bytes.restype = sz
    L.acm_gpu_sort_tmp_bytes.argtypes = [u64]
    L.acm_gpu_sort_records_device.restype = i32
    L.acm_gpu_sort_records_device.argtypes = [vp, vp, u64, vp, sz, vp]
    L.acm_gpu_order_tmp_bytes.restype = sz
    L.acm_gpu_order_tmp_bytes.argtypes = [vp, u64, u64]
    L.acm_gpu_order_records_device.restype = i32
    L.acm_gpu_order_records_device.argtypes = [vp, vp, u64, u64, u64, vp, sz, vp]
    L.acm_gpu_scan_ordered_tmp_bytes.restype = sz
    L.acm_gpu_scan_ordered_tmp_bytes.argtypes = [vp, u64, u64]
    L.acm_gpu_scan_ordered_device.restype = i32
    L.acm_gpu_scan_ordered_device.argtypes = [vp, vp, u64, u64, u64, vp, u64, vp, vp, sz, vp]
    L.acm_gpu_scan_host.restype = i32
    L.acm_gpu_scan_host.argtypes = [vp, vp, u64, u64, u64, vp, u64, C.POINTER(u64)]
    L.acm_scan.restype = i32
    L.acm_scan.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64)]
    L.acm_gpu_wire_bits.restype = i32
    L.acm_gpu_wire_bits.argtypes = [vp, u64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.acm_gpu_pack_records_device.restype = i32
    L.acm_gpu_pack_records_device.argtypes = [vp, u64, u64, C.c_uint32, C.c_uint32, vp, vp]
    L.acm_gpu_unpack_records_device.restype = i32
    L.acm_gpu_unpack_records_device.argtypes = [vp, u64, u64, C.c_uint32, C.c_uint32, vp, vp]
    L.acm_set_symbol_bytes.restype = i32
    L.acm_set_symbol_bytes.argtypes = [vp, C.c_uint32]
    L.acm_scan_path.restype = i32
    L.acm_scan_path.argtypes = [vp]
    L.acm_gpu_stream_open.restype = i32
    L.acm_gpu_stream_open.argtypes = [vp, u64, u64, C.POINTER(vp)]
    L.acm_gpu_stream_feed.restype = i32
    L.acm_gpu_stream_feed.argtypes = [vp, vp, u64]
    L.acm_gpu_stream_finish.restype = i32
    L.acm_gpu_stream_finish.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.acm_gpu_stream_close.restype = None
    L.acm_gpu_stream_close.argtypes = [vp]
    L.acm_gpu_plan_status.restype = i32
    L.acm_gpu_plan_status.argtypes = [vp]
    L.acm_gpu_plan_timing.restype = i32
    L.acm_gpu_plan_timing.argtypes = [vp, i32]
    L.acm_gpu_plan_timing_read.restype = i32
    L.acm_gpu_plan_timing_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(u64)]
    L.acm_gpu_multi_create.restype = i32
    L.acm_gpu_multi_create.argtypes = [vp, C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
    L.acm_gpu_multi_destroy.restype = None
    L.acm_gpu_multi_destroy.argtypes = [vp]
    L.acm_gpu_multi_shard_bounds.restype = i32
    L.acm_gpu_multi_shard_bounds.argtypes = [vp, u64, C.c_int, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.acm_gpu_multi_scan_host.restype = i32
    L.acm_gpu_multi_scan_host.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64)]
    L.acm_gpu_multi_scan_device.restype = i32
    L.acm_gpu_multi_scan_device.argtypes = [vp, C.POINTER(vp), u64, vp, u64, C.POINTER(u64)]
    L.acm_gpu_comm_unique_id.restype = i32
    L.acm_gpu_comm_unique_id.argtypes = [vp]
    L.acm_gpu_comm_init_rank.restype = i32
    L.acm_gpu_comm_init_rank.argtypes = [vp, i32, i32, C.POINTER(vp)]
    L.acm_gpu_comm_free.restype = i32
    L.acm_gpu_comm_free.argtypes = [vp]
    L.acm_gpu_comm_create.restype = i32
    L.acm_gpu_comm_create.argtypes = [vp, i32, i32, i32, C.POINTER(vp)]
    L.acm_gpu_comm_destroy.restype = None
    L.acm_gpu_comm_destroy.argtypes = [vp]
    L.acm_gpu_comm_gather_records.restype = i32
    L.acm_gpu_comm_gather_records.argtypes = [vp, vp, vp, u64, u64, u64, vp, u64, C.POINTER(u64), C.POINTER(u64), vp]
    L.acm_gpu_plan_timing_read_all.restype = i32
    L.acm_gpu_plan_timing_read_all.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(u64)]
    L.acm_gpu_scan_batch_tmp_bytes.restype = sz
    L.acm_gpu_scan_batch_tmp_bytes.argtypes = [vp, u64, u64, u64]
    L.acm_gpu_scan_batch_device.restype = i32
    L.acm_gpu_scan_batch_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, u64, vp, vp, sz, vp]
    L.acm_gpu_scan_batch_host.restype = i32
    L.acm_gpu_scan_batch_host.argtypes = [vp, vp, vp, u64, vp, vp, vp, u64, C.POINTER(u64)]
    L.acm_scan_batch.restype = i32
    L.acm_scan_batch.argtypes = [vp, vp, vp, u64, vp, vp, vp, u64, C.POINTER(u64)]
    L.acm_gpu_tally_tmp_bytes.restype = sz
    L.acm_gpu_tally_tmp_bytes.argtypes = [vp, u64, u64]
    L.acm_gpu_tally_device.restype = i32
    L.acm_gpu_tally_device.argtypes = [vp, vp, u64, u64, vp, u64, u64, u64, vp, vp, vp, sz, vp]
    L.acm_gpu_tally_form.restype = i32
    L.acm_gpu_tally_form.argtypes = [vp]
    L.acm_gpu_tally_keywords.restype = u64
    L.acm_gpu_tally_keywords.argtypes = [vp]
    L.acm_gpu_tally_host.restype = i32
    L.acm_gpu_tally_host.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64)]
    L.acm_tally.restype = i32
    L.acm_tally.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64)]
    L.acm_select_records.restype = u64
    L.acm_select_records.argtypes = [vp, u64]
    L.acm_gpu_select_tmp_bytes.restype = sz
    L.acm_gpu_select_tmp_bytes.argtypes = [vp, u64, u64]
    L.acm_gpu_select_records_device.restype = i32
    L.acm_gpu_select_records_device.argtypes = [vp, vp, u64, vp, u64, u64, vp, vp, vp, sz, vp]
    L.acm_gpu_select_form.restype = i32
    L.acm_gpu_select_form.argtypes = [vp]
    L.acm_gpu_scan_select_tmp_bytes.restype = sz
    L.acm_gpu_scan_select_tmp_bytes.argtypes = [vp, u64, u64]
    L.acm_gpu_scan_select_device.restype = i32
    L.acm_gpu_scan_select_device.argtypes = [vp, vp, u64, u64, vp, u64, vp, vp, sz, vp]
    L.acm_gpu_scan_select_host.restype = i32
    L.acm_gpu_scan_select_host.argtypes = [vp, vp, u64, u64, vp, u64, C.POINTER(u64)]
    L.acm_select.restype = i32
    L.acm_select.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64)]
    L.acm_score_check.restype = i32
    L.acm_score_check.argtypes = [vp, vp, vp, vp, u64, u64]
    L.acm_score_matrix.restype = i32
    L.acm_score_matrix.argtypes = [vp, vp, vp, u64, u64, vp, vp, vp, vp, u64, vp, vp, vp, u64, C.POINTER(u64), vp]
    L.acm_score_top.restype = i32
    L.acm_score_top.argtypes = [vp, vp, vp, u64, u64, u32, vp, vp, vp, vp]
    L.acm_gpu_score_create.restype = i32
    L.acm_gpu_score_create.argtypes = [vp, vp, vp, vp, vp, u64, C.POINTER(vp)]
    L.acm_gpu_score_destroy.restype = None
    L.acm_gpu_score_destroy.argtypes = [vp]
    L.acm_gpu_score_info.restype = i32
    L.acm_gpu_score_info.argtypes = [vp, C.POINTER(ScoreInfo)]
    L.acm_gpu_score_matrix_tmp_bytes.restype = sz
    L.acm_gpu_score_matrix_tmp_bytes.argtypes = [vp, vp, u64]
    L.acm_gpu_score_matrix_device.restype = i32
    L.acm_gpu_score_matrix_device.argtypes = [vp, vp, vp, vp, vp, u64, vp, vp, vp, u64, vp, vp, vp, sz, vp]
    L.acm_gpu_score_top_tmp_bytes.restype = sz
    L.acm_gpu_score_top_tmp_bytes.argtypes = [vp, u64, u64]
    L.acm_gpu_score_top_device.restype = i32
    L.acm_gpu_score_top_device.argtypes = [vp, vp, vp, vp, u64, u64, u64, u32, vp, vp, vp, vp, vp, sz, vp]
    L.acm_gpu_score_tmp_bytes.restype = sz
    L.acm_gpu_score_tmp_bytes.argtypes = [vp, vp, u64, u64, u64, u64, u64, u64, u32]
    L.acm_gpu_score_device.restype = i32
    L.acm_gpu_score_device.argtypes = [vp, vp, vp, u64, vp, u64, u64, u64, u64, vp, vp, vp, u64, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    for fn in (L.acm_gpu_score_host, L.acm_score):
        fn.restype = i32
        fn.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, u64, vp, vp, vp, u64, C.POINTER(u64), vp, u32, vp, vp, vp, vp, C.POINTER(u64)]
    L.acm_index_matrix.restype = i32
    L.acm_index_matrix.argtypes = [vp, vp, vp, u64, u64, u64, vp, vp, vp, u64, C.POINTER(u64)]
    L.acm_index_concat.restype = i32
    L.acm_index_concat.argtypes = [vp, vp, vp, u64, vp, vp, vp, u64, vp, vp, vp, u64, C.POINTER(u64)]
    L.acm_gpu_index_matrix_tmp_bytes.restype = sz
    L.acm_gpu_index_matrix_tmp_bytes.argtypes = [vp, u64, u64, u64]
    L.acm_gpu_index_matrix_device.restype = i32
    L.acm_gpu_index_matrix_device.argtypes = [vp, vp, vp, vp, u64, u64, u64, vp, vp, vp, u64, vp, vp, vp, sz, vp]
    L.acm_gpu_index_concat_tmp_bytes.restype = sz
    L.acm_gpu_index_concat_tmp_bytes.argtypes = [vp, u64]
    L.acm_gpu_index_concat_device.restype = i32
    L.acm_gpu_index_concat_device.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, u64, vp, vp, vp, u64, vp, vp, sz, vp]
    L.acm_gpu_index_tmp_bytes.restype = sz
    L.acm_gpu_index_tmp_bytes.argtypes = [vp, u64, u64, u64, u64, u64, u64, u64]
    L.acm_gpu_index_device.restype = i32
    L.acm_gpu_index_device.argtypes = [vp, vp, u64, vp, u64, u64, u64, u64, u64, u64, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, sz, vp]
    for fn in (L.acm_gpu_index_host, L.acm_index):
        fn.restype = i32
        fn.argtypes = [vp, vp, vp, u64, u64, vp, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.acm_cooccur_matrix.restype = i32
    L.acm_cooccur_matrix.argtypes = [vp, vp, vp, u64, u64, u32, u64, vp, vp, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.acm_cooccur_add.restype = i32
    L.acm_cooccur_add.argtypes = [vp, vp, vp, u64, vp, vp, vp, u64, vp, vp, vp, u64, C.POINTER(u64)]
    L.acm_gpu_cooccur_matrix_tmp_bytes.restype = sz
    L.acm_gpu_cooccur_matrix_tmp_bytes.argtypes = [vp, u64, u64, u64]
    L.acm_gpu_cooccur_matrix_device.restype = i32
    L.acm_gpu_cooccur_matrix_device.argtypes = [vp, vp, vp, vp, u64, u64, u32, u64, u64, vp, vp, vp, u64, vp, vp, vp, vp, sz, vp]
    L.acm_gpu_cooccur_add_tmp_bytes.restype = sz
    L.acm_gpu_cooccur_add_tmp_bytes.argtypes = [vp, u64, u64]
    L.acm_gpu_cooccur_add_device.restype = i32
    L.acm_gpu_cooccur_add_device.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, u64, u64, vp, vp, vp, u64, vp, vp, vp, sz, vp]
    L.acm_gpu_cooccur_tmp_bytes.restype = sz
    L.acm_gpu_cooccur_tmp_bytes.argtypes = [vp, u64, u64, u64, u64, u64, u64, u64]
    L.acm_gpu_cooccur_device.restype = i32
    L.acm_gpu_cooccur_device.argtypes = [vp, vp, u64, vp, u64, u64, u64, u64, u64, u32, u64, u64, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    for fn in (L.acm_gpu_cooccur_host, L.acm_cooccur):
        fn.restype = i32
        fn.argtypes = [vp, vp, vp, u64, u64, u32, u64, vp, vp, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.acm_segment_records.restype = i32
    L.acm_segment_records.argtypes = [vp, u64, vp, u64, u32, C.POINTER(u64), vp]
    L.acm_gpu_segment_tmp_bytes.restype = sz
    L.acm_gpu_segment_tmp_bytes.argtypes = [vp, u64, u64]
    L.acm_gpu_segment_records_device.restype = i32
    L.acm_gpu_segment_records_device.argtypes = [vp, vp, u64, vp, u64, u64, vp, u64, u32, vp, vp, vp, vp, sz, vp]
    L.acm_gpu_scan_segment_tmp_bytes.restype = sz
    L.acm_gpu_scan_segment_tmp_bytes.argtypes = [vp, u64, u64, u64]
    L.acm_gpu_scan_segment_device.restype = i32
    L.acm_gpu_scan_segment_device.argtypes = [vp, vp, u64, u64, vp, u64, vp, u64, u32, vp, u64, vp, vp, vp, sz, vp]
    L.acm_gpu_scan_segment_host.restype = i32
    L.acm_gpu_scan_segment_host.argtypes = [vp, vp, u64, u64, vp, u64, vp, u64, u32, vp, u64, C.POINTER(u64), vp]
    L.acm_segment.restype = i32
    L.acm_segment.argtypes = [vp, vp, u64, vp, u64, u32, vp, u64, C.POINTER(u64), vp]
    L.acm_replace_records.restype = i32
    L.acm_replace_records.argtypes = [vp, u64, u32, u64, vp, u64, vp, vp, u64, vp, u64, C.POINTER(u64)]
    L.acm_gpu_replace_tmp_bytes.restype = sz
    L.acm_gpu_replace_tmp_bytes.argtypes = [vp, u64, u64]
    L.acm_gpu_replace_records_device.restype = i32
    L.acm_gpu_replace_records_device.argtypes = [vp, vp, u64, u64, vp, u64, vp, vp, vp, u64, vp, u64, vp, vp, vp, sz, vp]
    L.acm_gpu_scan_replace_tmp_bytes.restype = sz
    L.acm_gpu_scan_replace_tmp_bytes.argtypes = [vp, u64, u64]
    L.acm_gpu_scan_replace_device.restype = i32
    L.acm_gpu_scan_replace_device.argtypes = [vp, vp, u64, u64, vp, u64, vp, vp, vp, u64, vp, u64, vp, vp, vp, sz, vp]
    L.acm_gpu_scan_replace_host.restype = i32
    L.acm_gpu_scan_replace_host.argtypes = [vp, vp, u64, vp, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.acm_replace.restype = i32
    L.acm_replace.argtypes = [vp, vp, u64, vp, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.acm_tokens_records.restype = i32
    L.acm_tokens_records.argtypes = [vp, u64, u32, u64, vp, u64, vp, u64, vp, u64, u32, u32, vp, vp, vp, u64, C.POINTER(u64), vp]
    L.acm_gpu_tokens_tmp_bytes.restype = sz
    L.acm_gpu_tokens_tmp_bytes.argtypes = [vp, u64, u64]
    L.acm_gpu_tokens_records_device.restype = i32
    L.acm_gpu_tokens_records_device.argtypes = [vp, vp, u64, u64, vp, u64, vp, vp, u64, vp, u64, u32, u32, vp, vp, vp, u64, vp, vp, vp, sz, vp]
    L.acm_gpu_scan_tokens_tmp_bytes.restype = sz
    L.acm_gpu_scan_tokens_tmp_bytes.argtypes = [vp, u64, u64, u64]
    L.acm_gpu_scan_tokens_device.restype = i32
    L.acm_gpu_scan_tokens_device.argtypes = [vp, vp, u64, u64, vp, u64, vp, u64, vp, vp, u64, u32, u32, vp, vp, vp, u64, vp, vp, vp, sz, vp]
    L.acm_gpu_scan_tokens_host.restype = i32
    L.acm_gpu_scan_tokens_host.argtypes = [vp, vp, u64, vp, u64, vp, u64, u32, u32, vp, vp, vp, u64, C.POINTER(u64), vp, C.POINTER(u64)]
    L.acm_tokenize.restype = i32
    L.acm_tokenize.argtypes = [vp, vp, u64, vp, u64, vp, u64, u32, u32, vp, vp, vp, u64, C.POINTER(u64), vp, C.POINTER(u64)]
    L.acm_grep_gather.restype = i32
    L.acm_grep_gather.argtypes = [vp, u32, vp, u64, vp, u32, vp, C.POINTER(u64), vp, u64, vp, C.POINTER(u64)]
    L.acm_gpu_grep_tmp_bytes.restype = sz
    L.acm_gpu_grep_tmp_bytes.argtypes = [vp, u64, u64, u64, u64]
    L.acm_gpu_grep_device.restype = i32
    L.acm_gpu_grep_device.argtypes = [vp, vp, u64, vp, u64, u32, u64, u64, vp, vp, vp, vp, vp, vp, u64, vp, vp, vp, sz, vp]
    L.acm_gpu_grep_host.restype = i32
    L.acm_gpu_grep_host.argtypes = [vp, vp, vp, u64, u32, vp, vp, C.POINTER(u64), C.POINTER(u64), vp, u64, vp, C.POINTER(u64)]
    L.acm_grep.restype = i32
    L.acm_grep.argtypes = [vp, vp, vp, u64, u32, vp, vp, C.POINTER(u64), C.POINTER(u64), vp, u64, vp, C.POINTER(u64)]
    L.acm_tally_batch_records.restype = i32
    L.acm_tally_batch_records.argtypes = [vp, vp, u64, u64, vp, vp, vp, u64, C.POINTER(u64)]
    L.acm_gpu_tally_batch_tmp_bytes.restype = sz
    L.acm_gpu_tally_batch_tmp_bytes.argtypes = [vp, u64, u64, u64, u64, u64]
    L.acm_gpu_tally_batch_device.restype = i32
    L.acm_gpu_tally_batch_device.argtypes = [vp, vp, u64, vp, u64, u64, u64, u64, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.acm_gpu_tally_batch_host.restype = i32
    L.acm_gpu_tally_batch_host.argtypes = [vp, vp, vp, u64, vp, vp, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.acm_tally_batch.restype = i32
    L.acm_tally_batch.argtypes = [vp, vp, vp, u64, vp, vp, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.acm_rules_check.restype = i32
    L.acm_rules_check.argtypes = [vp, vp, vp, u64, u64]
    L.acm_rules_matrix.restype = i32
    L.acm_rules_matrix.argtypes = [vp, vp, vp, u64, u64, vp, vp, vp, u64, vp, vp, u64, C.POINTER(u64)]
    L.acm_gpu_rules_create.restype = i32
    L.acm_gpu_rules_create.argtypes = [vp, vp, vp, vp, u64, C.POINTER(vp)]
    L.acm_gpu_rules_destroy.restype = None
    L.acm_gpu_rules_destroy.argtypes = [vp]
    L.acm_gpu_rules_info.restype = i32
    L.acm_gpu_rules_info.argtypes = [vp, C.POINTER(RulesInfo)]
    L.acm_gpu_rules_matrix_tmp_bytes.restype = sz
    L.acm_gpu_rules_matrix_tmp_bytes.argtypes = [vp, vp, u64]
    L.acm_gpu_rules_matrix_device.restype = i32
    L.acm_gpu_rules_matrix_device.argtypes = [vp, vp, vp, vp, vp, u64, vp, vp, u64, vp, vp, sz, vp]
    L.acm_gpu_rules_tmp_bytes.restype = sz
    L.acm_gpu_rules_tmp_bytes.argtypes = [vp, vp, u64, u64, u64, u64, u64]
    L.acm_gpu_rules_device.restype = i32
    L.acm_gpu_rules_device.argtypes = [vp, vp, vp, u64, vp, u64, u64, u64, u64, vp, vp, u64, vp, vp, vp, vp, vp, sz, vp]
    for fn in (L.acm_gpu_rules_host, L.acm_rules):
        fn.restype = i32
        fn.argtypes = [vp, vp, vp, u64, vp, vp, vp, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.acm_patterns_check.restype = i32
    L.acm_patterns_check.argtypes = [vp, vp, u64, u64]
    L.acm_patterns_records.restype = i32
    L.acm_patterns_records.argtypes = [vp, u64, u64, u64, vp, u64, vp, vp, u64, u64, vp, u64, C.POINTER(u64)]
    L.acm_gpu_patterns_create.restype = i32
    L.acm_gpu_patterns_create.argtypes = [vp, vp, vp, u64, C.POINTER(vp)]
    L.acm_gpu_patterns_destroy.restype = None
    L.acm_gpu_patterns_destroy.argtypes = [vp]
    L.acm_gpu_patterns_info.restype = i32
    L.acm_gpu_patterns_info.argtypes = [vp, C.POINTER(PatternsInfo)]
    L.acm_gpu_patterns_tmp_bytes.restype = sz
    L.acm_gpu_patterns_tmp_bytes.argtypes = [vp, vp, u64, u64]
    L.acm_gpu_patterns_records_device.restype = i32
    L.acm_gpu_patterns_records_device.argtypes = [vp, vp, vp, u64, vp, u64, u64, vp, u64, vp, u64, vp, vp, sz, vp]
    L.acm_gpu_scan_patterns_tmp_bytes.restype = sz
    L.acm_gpu_scan_patterns_tmp_bytes.argtypes = [vp, vp, u64, u64, u64]
    L.acm_gpu_scan_patterns_device.restype = i32
    L.acm_gpu_scan_patterns_device.argtypes = [vp, vp, vp, u64, u64, vp, u64, u64, vp, u64, vp, vp, vp, sz, vp]
    L.acm_gpu_scan_patterns_host.restype = i32
    L.acm_gpu_scan_patterns_host.argtypes = [vp, vp, u64, u64, vp, u64, vp, vp, u64, vp, u64, C.POINTER(u64)]
    L.acm_scan_patterns.restype = i32
    L.acm_scan_patterns.argtypes = [vp, vp, u64, vp, u64, vp, vp, u64, vp, u64, C.POINTER(u64)]
    L.acm_chains_check.restype = i32
    L.acm_chains_check.argtypes = [vp, vp, u64, u64]
    L.acm_chains_records.restype = i32
    L.acm_chains_records.argtypes = [vp, u64, u64, u64, vp, u64, vp, vp, u64, u64, vp, u64, C.POINTER(u64)]
    L.acm_gpu_chains_create.restype = i32
    L.acm_gpu_chains_create.argtypes = [vp, vp, vp, u64, C.POINTER(vp)]
    L.acm_gpu_chains_destroy.restype = None
    L.acm_gpu_chains_destroy.argtypes = [vp]
    L.acm_gpu_chains_info.restype = i32
    L.acm_gpu_chains_info.argtypes = [vp, C.POINTER(ChainsInfo)]
    L.acm_gpu_chains_tmp_bytes.restype = sz
    L.acm_gpu_chains_tmp_bytes.argtypes = [vp, vp, u64, u64]
    L.acm_gpu_chains_records_device.restype = i32
    L.acm_gpu_chains_records_device.argtypes = [vp, vp, vp, u64, vp, u64, u64, vp, u64, vp, u64, vp, vp, sz, vp]
    L.acm_gpu_scan_chains_tmp_bytes.restype = sz
    L.acm_gpu_scan_chains_tmp_bytes.argtypes = [vp, vp, u64, u64, u64]
    L.acm_gpu_scan_chains_device.restype = i32
    L.acm_gpu_scan_chains_device.argtypes = [vp, vp, vp, u64, u64, vp, u64, u64, vp, u64, vp, vp, vp, sz, vp]
    L.acm_gpu_scan_chains_host.restype = i32
    L.acm_gpu_scan_chains_host.argtypes = [vp, vp, u64, u64, vp, u64, vp, vp, u64, vp, u64, C.POINTER(u64)]
    L.acm_scan_chains.restype = i32
    L.acm_scan_chains.argtypes = [vp, vp, u64, vp, u64, vp, vp, u64, vp, u64, C.POINTER(u64)]
    L.acm_near_check.restype = i32
    L.acm_near_check.argtypes = [vp, vp, vp, u64, u64]
    L.acm_near_records.restype = i32
    L.acm_near_records.argtypes = [vp, u64, u64, u64, vp, u64, vp, vp, vp, u64, u64, vp, u64, C.POINTER(u64)]
    L.acm_gpu_near_create.restype = i32
    L.acm_gpu_near_create.argtypes = [vp, vp, vp, vp, u64, C.POINTER(vp)]
    L.acm_gpu_near_destroy.restype = None
    L.acm_gpu_near_destroy.argtypes = [vp]
    L.acm_gpu_near_info.restype = i32
    L.acm_gpu_near_info.argtypes = [vp, C.POINTER(NearInfo)]
    L.acm_gpu_near_tmp_bytes.restype = sz
    L.acm_gpu_near_tmp_bytes.argtypes = [vp, vp, u64, u64]
    L.acm_gpu_near_records_device.restype = i32
    L.acm_gpu_near_records_device.argtypes = [vp, vp, vp, u64, vp, u64, u64, vp, u64, vp, u64, vp, vp, sz, vp]
    L.acm_gpu_scan_near_tmp_bytes.restype = sz
    L.acm_gpu_scan_near_tmp_bytes.argtypes = [vp, vp, u64, u64, u64]
    L.acm_gpu_scan_near_device.restype = i32
    L.acm_gpu_scan_near_device.argtypes = [vp, vp, vp, u64, u64, vp, u64, u64, vp, u64, vp, vp, vp, sz, vp]
    L.acm_gpu_scan_near_host.restype = i32
    L.acm_gpu_scan_near_host.argtypes = [vp, vp, u64, u64, vp, u64, vp, vp, vp, u64, vp, u64, C.POINTER(u64)]
    L.acm_scan_near.restype = i32
    L.acm_scan_near.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, u64, vp, u64, C.POINTER(u64)]
    L.acm_approx_check.restype = i32
    L.acm_approx_check.argtypes = [vp, vp, vp, vp, u64, u64]
    L.acm_approx_split.restype = i32
    L.acm_approx_split.argtypes = [u64, u32, u32, C.POINTER(u64), C.POINTER(u64)]
    L.acm_approx_records.restype = i32
    L.acm_approx_records.argtypes = [vp, u64, vp, u32, u64, u64, vp, u64, vp, vp, vp, vp, vp, u64, u64, vp, vp, u64, C.POINTER(u64)]
    L.acm_gpu_approx_create.restype = i32
    L.acm_gpu_approx_create.argtypes = [vp, vp, vp, vp, vp, vp, u64, C.POINTER(vp)]
    L.acm_gpu_approx_destroy.restype = None
    L.acm_gpu_approx_destroy.argtypes = [vp]
    L.acm_gpu_approx_info.restype = i32
    L.acm_gpu_approx_info.argtypes = [vp, C.POINTER(ApproxInfo)]
    L.acm_gpu_approx_tmp_bytes.restype = sz
    L.acm_gpu_approx_tmp_bytes.argtypes = [vp, vp, u64, u64, u64]
    L.acm_gpu_approx_records_device.restype = i32
    L.acm_gpu_approx_records_device.argtypes = [vp, vp, vp, u64, vp, vp, u64, u64, vp, u64, vp, vp, u64, vp, vp, sz, vp]
    L.acm_gpu_scan_approx_tmp_bytes.restype = sz
    L.acm_gpu_scan_approx_tmp_bytes.argtypes = [vp, vp, u64, u64, u64, u64]
    L.acm_gpu_scan_approx_device.restype = i32
    L.acm_gpu_scan_approx_device.argtypes = [vp, vp, vp, u64, u64, vp, u64, u64, vp, vp, u64, vp, vp, vp, sz, vp]
    L.acm_gpu_scan_approx_host.restype = i32
    L.acm_gpu_scan_approx_host.argtypes = [vp, vp, u64, u64, vp, u64, vp, vp, vp, vp, vp, u64, vp, vp, u64, C.POINTER(u64)]
    L.acm_scan_approx.restype = i32
    L.acm_scan_approx.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, vp, vp, u64, vp, vp, u64, C.POINTER(u64)]
    L.acm_templates_check.restype = i32
    L.acm_templates_check.argtypes = [vp, u32, u64]
    L.acm_templates_split.restype = i32
    L.acm_templates_split.argtypes = [vp, u64, u32, u32, C.POINTER(u64), C.POINTER(u64)]
    L.acm_templates_records.restype = i32
    L.acm_templates_records.argtypes = [vp, u64, vp, u32, u64, u64, vp, u64, vp, u64, vp, vp, u64, C.POINTER(u64)]
    L.acm_gpu_templates_create.restype = i32
    L.acm_gpu_templates_create.argtypes = [vp, vp, C.POINTER(vp)]
    L.acm_gpu_templates_destroy.restype = None
    L.acm_gpu_templates_destroy.argtypes = [vp]
    L.acm_gpu_templates_info.restype = i32
    L.acm_gpu_templates_info.argtypes = [vp, C.POINTER(TemplatesInfo)]
    for call in ("acm_gpu_%s_tmp_bytes", "acm_gpu_%s_records_device", "acm_gpu_scan_%s_tmp_bytes", "acm_gpu_scan_%s_device"):   # APPROX's signatures
        getattr(L, call % "templates").restype = getattr(L, call % "approx").restype
        getattr(L, call % "templates").argtypes = getattr(L, call % "approx").argtypes
    L.acm_gpu_scan_templates_host.restype = i32
    L.acm_gpu_scan_templates_host.argtypes = [vp, vp, u64, u64, vp, u64, vp, vp, vp, u64, C.POINTER(u64)]
    L.acm_scan_templates.restype = i32
    L.acm_scan_templates.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, u64, C.POINTER(u64)]
    for call in ("acm_%s_check", "acm_%s_records", "acm_gpu_%s_tmp_bytes", "acm_gpu_%s_records_device", "acm_gpu_scan_%s_tmp_bytes",
                 "acm_gpu_scan_%s_device", "acm_gpu_scan_%s_host", "acm_scan_%s"):   # the edit calls have the signatures of their APPROX counterparts
        getattr(L, call % "edit").restype = getattr(L, call % "approx").restype
        getattr(L, call % "edit").argtypes = getattr(L, call % "approx").argtypes
    L.acm_split_offsets.restype = i32
    L.acm_split_offsets.argtypes = [vp, u64, u32, vp, u32, u32, vp, u64, C.POINTER(u64)]
    L.acm_gpu_split_tmp_bytes.restype = sz
    L.acm_gpu_split_tmp_bytes.argtypes = [vp, u64]
    L.acm_gpu_split_device.restype = i32
    L.acm_gpu_split_device.argtypes = [vp, vp, u64, vp, u32, u32, vp, u64, vp, vp, sz, vp]
    L.acm_gpu_split_host.restype = i32
    L.acm_gpu_split_host.argtypes = [vp, vp, u64, vp, u32, u32, vp, u64, C.POINTER(u64)]
    for fn in (L.acm_gpu_grep_lines_host, L.acm_grep_lines):
        fn.restype = i32
        fn.argtypes = [vp, vp, u64, vp, u32, u32, u32, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp, u64, C.POINTER(u64), u64, vp, vp, vp, vp]
    L.acm_words_records.restype = i32
    L.acm_words_records.argtypes = [vp, u64, u32, u64, vp, u64, vp, u32, u32, vp, u64, C.POINTER(u64)]
    L.acm_gpu_words_tmp_bytes.restype = sz
    L.acm_gpu_words_tmp_bytes.argtypes = [vp, u64, u64]
    L.acm_gpu_words_records_device.restype = i32
    L.acm_gpu_words_records_device.argtypes = [vp, vp, u64, u64, vp, u64, vp, u32, u32, vp, u64, vp, vp, vp, vp, sz, vp]
    L.acm_gpu_scan_words_tmp_bytes.restype = sz
    L.acm_gpu_scan_words_tmp_bytes.argtypes = [vp, u64, u64, u64]
    L.acm_gpu_scan_words_device.restype = i32
    L.acm_gpu_scan_words_device.argtypes = [vp, vp, u64, u64, vp, u64, vp, u32, u32, vp, u64, vp, vp, sz, vp]
    L.acm_gpu_scan_words_host.restype = i32
    L.acm_gpu_scan_words_host.argtypes = [vp, vp, u64, u64, vp, u64, vp, u32, u32, vp, u64, C.POINTER(u64)]
    L.acm_scan_words.restype = i32
    L.acm_scan_words.argtypes = [vp, vp, u64, vp, u32, u32, vp, u64, C.POINTER(u64)]
    ctx_out = [vp, u64, C.POINTER(u64), C.POINTER(u64), vp, vp, vp, vp, vp]   # out, out_capacity, out_symbols, n_snippets, the five arrays
    L.acm_context_records.restype = i32
    L.acm_context_records.argtypes = [vp, u64, u32, u64, vp, u64, vp, u64, u32, u32, u32] + ctx_out
    L.acm_gpu_context_tmp_bytes.restype = sz
    L.acm_gpu_context_tmp_bytes.argtypes = [vp, u64, u64]
    L.acm_gpu_context_records_device.restype = i32
    L.acm_gpu_context_records_device.argtypes = [vp, vp, u64, u64, vp, u64, vp, u64, vp, u32, u32, u32, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.acm_gpu_scan_context_tmp_bytes.restype = sz
    L.acm_gpu_scan_context_tmp_bytes.argtypes = [vp, u64, u64, u64]
    L.acm_gpu_scan_context_device.restype = i32
    L.acm_gpu_scan_context_device.argtypes = [vp, vp, u64, u64, vp, u64, vp, u64, vp, u32, u32, u32, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.acm_gpu_scan_context_host.restype = i32
    L.acm_gpu_scan_context_host.argtypes = [vp, vp, u64, u64, vp, u64, vp, u64, C.POINTER(u64), u32, u32, u32] + ctx_out
    L.acm_context.restype = i32
    L.acm_context.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64), u32, u32, u32] + ctx_out
    L.acm_anchored_records.restype = i32
    L.acm_anchored_records.argtypes = [vp, u64, u32, vp, u64, vp, vp, C.POINTER(u64)]
    L.acm_gpu_scan_anchored_tmp_bytes.restype = sz
    L.acm_gpu_scan_anchored_tmp_bytes.argtypes = [vp, u64]
    L.acm_gpu_scan_anchored_device.restype = i32
    L.acm_gpu_scan_anchored_device.argtypes = [vp, vp, u64, vp, u64, u32, vp, vp, vp, u64, vp, vp, sz, vp]
    L.acm_gpu_lookup_tmp_bytes.restype = sz
    L.acm_gpu_lookup_tmp_bytes.argtypes = [vp, u64]
    L.acm_gpu_lookup_device.restype = i32
    L.acm_gpu_lookup_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, vp, sz, vp]
    L.acm_gpu_scan_anchored_host.restype = i32
    L.acm_gpu_scan_anchored_host.argtypes = [vp, vp, vp, u64, u32, vp, vp, vp, u64, C.POINTER(u64)]
    L.acm_gpu_lookup_host.restype = i32
    L.acm_gpu_lookup_host.argtypes = [vp, vp, vp, u64, vp, vp, vp]
    L.acm_scan_anchored.restype = i32
    L.acm_scan_anchored.argtypes = [vp, vp, vp, u64, u32, vp, vp, vp, u64, C.POINTER(u64)]
    L.acm_lookup.restype = i32
    L.acm_lookup.argtypes = [vp, vp, vp, u64, vp, vp, vp]
    L.acm_gpu_flows_create.restype = i32
    L.acm_gpu_flows_create.argtypes = [vp, u64, C.POINTER(vp)]
    L.acm_gpu_flows_destroy.restype = None
    L.acm_gpu_flows_destroy.argtypes = [vp]
    L.acm_gpu_flows_reset.restype = i32
    L.acm_gpu_flows_reset.argtypes = [vp, vp, u64, vp]
    L.acm_gpu_scan_flows_tmp_bytes.restype = sz
    L.acm_gpu_scan_flows_tmp_bytes.argtypes = [vp, vp, u64, u64, u64]
    L.acm_gpu_scan_flows_device.restype = i32
    L.acm_gpu_scan_flows_device.argtypes = [vp, vp, vp, u64, vp, vp, u64, vp, vp, vp, u64, vp, vp, sz, vp]
    L.acm_gpu_scan_flows_host.restype = i32
    L.acm_gpu_scan_flows_host.argtypes = [vp, vp, vp, u64, vp, vp, u64, vp, vp, vp, u64, C.POINTER(u64)]
    L.acm_scan_from.restype = i32
    L.acm_scan_from.argtypes = [vp, C.POINTER(vp), vp, u64, vp, u64, C.POINTER(u64)]
    L.acm_chars_positions.restype = i32
    L.acm_chars_positions.argtypes = [vp, u64, vp, u64, u32, vp, u64, vp]
    L.acm_chars_records.restype = i32
    L.acm_chars_records.argtypes = [vp, u64, u64, vp, u64, u32, vp, u64, vp, vp, vp]
    L.acm_gpu_chars_ruler_bytes.restype = sz
    L.acm_gpu_chars_ruler_bytes.argtypes = [vp, u64]
    L.acm_gpu_chars_ruler_tmp_bytes.restype = sz
    L.acm_gpu_chars_ruler_tmp_bytes.argtypes = [vp, u64]
    L.acm_gpu_chars_ruler_device.restype = i32
    L.acm_gpu_chars_ruler_device.argtypes = [vp, vp, u64, vp, sz, vp, sz, vp]
    L.acm_gpu_chars_tmp_bytes.restype = sz
    L.acm_gpu_chars_tmp_bytes.argtypes = [vp, u64, u64]
    L.acm_gpu_chars_records_device.restype = i32
    L.acm_gpu_chars_records_device.argtypes = [vp, vp, u64, u64, vp, u64, u32, vp, vp, u64, vp, vp, vp, vp, vp, sz, vp]
    L.acm_gpu_chars_positions_device.restype = i32
    L.acm_gpu_chars_positions_device.argtypes = [vp, vp, u64, vp, u64, u32, vp, vp, u64, vp, vp, sz, vp]
    L.acm_gpu_scan_chars_tmp_bytes.restype = sz
    L.acm_gpu_scan_chars_tmp_bytes.argtypes = [vp, u64, u64, u64]
    L.acm_gpu_scan_chars_device.restype = i32
    L.acm_gpu_scan_chars_device.argtypes = [vp, vp, u64, u64, vp, u64, u32, vp, vp, vp, vp, u64, vp, vp, sz, vp]
    L.acm_gpu_scan_chars_host.restype = i32
    L.acm_gpu_scan_chars_host.argtypes = [vp, vp, u64, u64, vp, u64, u32, vp, vp, vp, vp, u64, C.POINTER(u64)]
    L.acm_scan_chars.restype = i32
    L.acm_scan_chars.argtypes = [vp, vp, u64, u32, vp, vp, vp, vp, u64, C.POINTER(u64)]
    L.acm_gpu_synth_text.restype = i32
    L.acm_gpu_synth_text.argtypes = [i32, vp, u64, u64, u32, u32, vp, vp, u32, vp]
    _lib = L
    return L


def _check(rc, what):
    if rc != ACM_GPU_OK:
        raise ACMError(rc, what)


_SYM_DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def _ptr(a):
    """the address of a numpy array, None for an empty one"""
    return a.ctypes.data if a.size else None


def _opt(x):
    """the address of an optional numpy array or device tensor: None stays None"""
    if x is None:
        return None
    return x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data


def _opt_full(x):
    """the address of an optional device tensor that holds something: None for None and for an empty one"""
    return x.data_ptr() if x is not None and x.numel() else None


def _cut(offsets):
    """(address, n_texts) of the optional offsets of a batch -- a numpy array or a device tensor of n_texts + 1
    entries --, (None, 0) for a buffer that is one text"""
    return (_opt(offsets), offsets.shape[0] - 1) if offsets is not None else (None, 0)


def _room_call(call, what, cap, fixed=False, repeats=1):
    """The room loop of the host calls: call(cap) -> (rc, need, out) runs the C call with room for `cap`
    entries; on ACM_GPU_E_OVERFLOW it is repeated with `need`, the size the call reported -- `repeats` times
    at the most (None: until it fits), and never when the caller `fixed` the capacity.  Returns (out, need,
    cap) of the call that had room; any other outcome raises ACMError(rc, what)."""
    attempt = 0
    while True:
        rc, need, out = call(cap)
        if rc == ACM_GPU_E_OVERFLOW and not fixed and (repeats is None or attempt < repeats):
            cap, attempt = int(need), attempt + 1
            continue
        _check(rc, what)
        return out, int(need), cap


def _records_host_call(fn, what, before, cap, fixed, repeats=1):
    """fn(*before, out, cap, n) in the room loop, for the host calls that fill `cap` records and nothing else:
    the records"""
    def call(cap):
        out = np.zeros(cap, dtype=RECORD_DTYPE)
        n = C.c_uint64(0)
        return fn(*before, out.ctypes.data, cap, C.byref(n)), n.value, out
    out, n, _ = _room_call(call, what, cap, fixed, repeats)
    return out[:n]


def _matches_host_call(fn, what, before, out_capacity, extra=()):
    """fn(*before, out, one array per dtype of `extra`, cap, n) in the room loop, for the host calls of the
    pattern, chain, approx, edit and template families: room for 1024 matches unless out_capacity says
    otherwise, no address for no room.  Returns (matches, the extra arrays...), cut to size."""
    def call(cap):
        out = np.zeros(max(cap, 1), dtype=RECORD_DTYPE)
        more = [np.zeros(max(cap, 1), dtype=d) for d in extra]
        n = C.c_uint64(0)
        rc = fn(*before, out.ctypes.data if cap else None, *[m.ctypes.data for m in more], cap, C.byref(n))
        return rc, n.value, (out, *more)
    arrays, n, _ = _room_call(call, what, int(out_capacity) if out_capacity is not None else 1024, out_capacity is not None)
    return tuple(a[:n] for a in arrays)


def _counted(call, capacity, count):
    """call(capacity) when a capacity is given; None: call(0), which only counts, then call again sized by the
    count -- the attribute `count` of what call returns"""
    got = call(int(capacity) if capacity is not None else 0)
    if capacity is None and getattr(got, count):
        got = call(getattr(got, count))
    return got


def _device_room_call(run, what, cap):
    """run(cap) -> (count, out) for a device call whose count is read back: repeated once, sized by the count,
    when that is above cap.  Returns (count, out); ACMError (ACM_GPU_E_OVERFLOW) when it still has no room."""
    n, out = run(cap)
    if n > cap:
        cap = n
        n, out = run(cap)
        if n > cap:
            raise ACMError(ACM_GPU_E_OVERFLOW, "%s: %d records" % (what, n))
    return n, out


def _scratch(tb, dev, tmp=None):
    """a uint8 scratch tensor of tb bytes or more on `dev` (16 at the least: the calls want an address): the
    caller's `tmp` when that is large enough"""
    import torch
    if tmp is None or tmp.numel() < tb:
        tmp = torch.empty(max(tb, 16), dtype=torch.uint8, device=dev)
    return tmp


def _i64(n, dev):
    """a zeroed int64 tensor of n entries on `dev`: the numbers a device call leaves for the host"""
    import torch
    return torch.zeros(n, dtype=torch.int64, device=dev)


class _Owner:
    """An object over a native handle: whatever its close() releases goes with the object."""

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def select_records(array):
    """acm_select_records(): the leftmost-longest non-overlapping records of `array` (RECORD_DTYPE, in
    canonical order), by the sequential pass on the host.  Returns a new array; `array` is not changed."""
    a = np.array(array, dtype=RECORD_DTYPE, copy=True).reshape(-1)
    n = lib().acm_select_records(a.ctypes.data if a.size else None, a.size)
    return a[:n]


def _costs(cost):
    """a cost table as the segment calls take it: uint32, contiguous"""
    c = np.ascontiguousarray(cost, dtype=np.uint32).reshape(-1)
    return c, (c.ctypes.data if c.size else None)


def segment_records(array, cost, gap_cost):
    """acm_segment_records(): the minimum-cost tiling of `array` (RECORD_DTYPE, in canonical order) under
    cost[keyword_id] per record and gap_cost per uncovered symbol (include/acm_segment.h), by the
    sequential pass on the host.  Returns (records, sums): a new array, `array` is not changed; sums =
    (the cost of the records, their lengths)."""
    a = np.array(array, dtype=RECORD_DTYPE, copy=True).reshape(-1)
    c, cp = _costs(cost)
    n = C.c_uint64(0)
    sums = np.zeros(2, np.uint64)
    _check(lib().acm_segment_records(a.ctypes.data if a.size else None, a.size, cp, c.size, int(gap_cost), C.byref(n), sums.ctypes.data),
           "acm_segment_records")
    return a[:n.value], (int(sums[0]), int(sums[1]))


def replacement_table(replacements, sym_size, fill=None):
    """(repl_data, repl_off, n_keywords) of the replace calls.  `replacements`: one entry per keyword, in
    keyword_id order, each `bytes` (one symbol per byte, as Machine.add_keyword takes them; raw bytes
    for a symbol size numpy has no type for) or an array of symbols, possibly empty.  `fill`: ONE
    symbol instead (mask mode): repl_off is None then."""
    dtype = _SYM_DTYPE.get(sym_size, np.uint8)
    per = sym_size // np.dtype(dtype).itemsize                      # array entries per symbol
    assert (replacements is None) != (fill is None), "either replacements or fill"

    def symbols(x):
        if isinstance(x, (bytes, bytearray)):
            x = np.frombuffer(bytes(x), dtype=np.uint8)
        a = np.ascontiguousarray(x, dtype=dtype).reshape(-1)
        assert a.size % per == 0
        return a
    if fill is not None:
        one = symbols(fill) if isinstance(fill, (bytes, bytearray, np.ndarray, list, tuple)) else np.array([fill], dtype=dtype)
        assert one.size == per, "fill is one symbol"
        return one, None, 0
    parts = [symbols(r) for r in replacements]
    off = np.zeros(len(parts) + 1, np.uint64)
    if parts:
        np.cumsum([p.size // per for p in parts], out=off[1:])
    data = np.concatenate(parts + [np.zeros(per, dtype)])           # (never empty: the calls want an address)
    return data, off, len(parts)


def replace_records(text, records, replacements=None, fill=None, pos_base=0, sym_size=None, out_capacity=None):
    """acm_replace_records(): `text` (an array of symbols; with sym_size, raw bytes of symbols of that
    size) with every record of `records` (a selection: RECORD_DTYPE, canonical order, no two sharing a
    symbol) replaced by its keyword's entry of `replacements`, or masked with `fill`; the sequential
    pass on the host.  Returns the new array.  out_capacity (symbols; None: what the output needs)."""
    t = np.ascontiguousarray(text)
    sb = int(sym_size) if sym_size is not None else t.itemsize
    n_sym = t.size * t.itemsize // sb
    rec = np.ascontiguousarray(np.asarray(records, dtype=RECORD_DTYPE).reshape(-1))
    data, off, nk = replacement_table(replacements, sb, fill)
    need = C.c_uint64(0)

    def call(out, cap):
        return lib().acm_replace_records(_ptr(t), n_sym, sb, pos_base, _ptr(rec), rec.size, data.ctypes.data, _opt(off), nk, _opt(out), cap,
                                         C.byref(need))
    if out_capacity is None:
        rc = call(None, 0)
        if rc not in (ACM_GPU_OK, ACM_GPU_E_OVERFLOW):
            _check(rc, "acm_replace_records")
        out_capacity = int(need.value)
    out = np.zeros(max(int(out_capacity) * sb // t.itemsize, 1), dtype=t.dtype)
    _check(call(out, int(out_capacity)), "acm_replace_records")
    return out[:int(need.value) * sb // t.itemsize]


TOKENS_GAP_SYMBOL, TOKENS_GAP_RUN, TOKENS_GAP_DROP = 0, 1, 2
_TOKEN_MODES = {"symbol": TOKENS_GAP_SYMBOL, "run": TOKENS_GAP_RUN, "drop": TOKENS_GAP_DROP}


def _token_mode(mode):
    return _TOKEN_MODES[mode] if isinstance(mode, str) else int(mode)


class Tokens:
    """What the tokenising calls return.  ids (one vocabulary id per token), start (where every token
    begins, in the records' coordinate), length (its symbols) and first (n_texts + 1 row pointers:
    tokens [first[t], first[t + 1]) are those of text t; None when the buffer was one text): int32 /
    int64 / int32 / int64 device tensors with room for token_capacity entries from Plan.tokens_records()
    and Plan.scan_tokens() -- the first n_tokens count --, uint32 / uint64 / uint32 / uint64 numpy arrays
    cut to size from the host calls.  n_tokens and count are Python ints (the device calls synchronise to
    read them): n_tokens > token_capacity is the room the tokens need (ids, start and length are
    unspecified then, first is valid), count > the record capacity the room the records need (n_tokens
    is 0 then).  records is the selection (int64 [capacity, 2], device calls only), count its size."""

    def __init__(self, ids, start, length, first, n_tokens, records=None, count=None, token_capacity=None):
        self.ids, self.start, self.length, self.first, self.n_tokens = ids, start, length, first, n_tokens
        self.records, self.count, self.token_capacity = records, count, token_capacity

    def padded(self, pad_id):
        """The ragged rows as one n_texts x max_len int64 tensor on the device the ids are on (numpy
        arrays go to the current device first), short rows filled with pad_id; built by torch from ids
        and first."""
        import torch
        assert self.first is not None, "padded() is for a batch"

        def tensor(a, dtype):
            if isinstance(a, torch.Tensor):
                return a
            return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).cuda()
        ids = tensor(self.ids, np.int32)[:self.n_tokens].view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        first = tensor(self.first, np.int64).view(torch.int64)
        lens = first[1:] - first[:-1]
        n_texts = lens.numel()
        width = int(lens.max().item()) if n_texts else 0
        out = torch.full((n_texts, width), int(pad_id), dtype=torch.int64, device=ids.device)
        if self.n_tokens:
            row = torch.repeat_interleave(torch.arange(n_texts, device=ids.device), lens)
            col = torch.arange(self.n_tokens, device=ids.device) - first[row]
            out[row, col] = ids
        return out


def _tok_of(tok_of):
    if tok_of is None:
        return None, 0
    a = np.ascontiguousarray(tok_of, dtype=np.uint32).reshape(-1)
    return (a if a.size else np.zeros(1, np.uint32)), int(np.asarray(tok_of).size)


def _tokens_host_call(call, what, n_texts, offsets_given, token_capacity):
    """the two-call pattern of the host entries: count (tok_id NULL), then fill.  call (ids, start,
    length, capacity, n_tokens, first, n_selected) -> rc"""
    first = np.zeros(n_texts + 1, np.uint64) if offsets_given else None
    need, m = C.c_uint64(0), C.c_uint64(0)
    if token_capacity is None:
        _check(call(None, None, None, 0, need, first, m), what)
        token_capacity = int(need.value)
    cap = int(token_capacity)
    ids, start, length = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1), np.uint32)
    _check(call(ids, start, length, cap, need, first, m), what)
    k = int(need.value)
    return Tokens(ids[:k], start[:k], length[:k], first, k, None, int(m.value), cap)


def tokens_records(text, records, offsets=None, mode="run", gap_base=0, tok_of=None, pos_base=0, sym_size=None, token_capacity=None):
    """acm_tokens_records(): the token stream of `text` (an array of symbols; with sym_size, raw bytes
    of symbols of that size; may be None in "run" and "drop" mode when sym_size and n_symbols =
    offsets[-1] say enough) under the selection `records` (RECORD_DTYPE, canonical order, no two
    sharing a symbol), by the sequential pass on the host.  `offsets` (n_texts + 1 entries) makes the
    buffer a batch.  Returns a Tokens of numpy arrays."""
    t = np.ascontiguousarray(text)
    sb = int(sym_size) if sym_size is not None else t.itemsize
    n_sym = t.size * t.itemsize // sb
    rec = np.ascontiguousarray(np.asarray(records, dtype=RECORD_DTYPE).reshape(-1))
    off = np.ascontiguousarray(offsets, dtype=np.uint64) if offsets is not None else None
    n_texts = off.size - 1 if off is not None else 0
    table, nk = _tok_of(tok_of)
    md = _token_mode(mode)

    def call(ids, start, length, cap, need, first, m):
        m.value = rec.size
        return lib().acm_tokens_records(_ptr(t), n_sym, sb, pos_base, _ptr(rec), rec.size, _opt(off), n_texts, _opt(table), nk, int(gap_base), md,
                                        _opt(ids), _opt(start), _opt(length), cap, C.byref(need), _opt(first))
    return _tokens_host_call(call, "acm_tokens_records", n_texts, off is not None, token_capacity)


class Grepped:
    """What the grep calls return.  hits (one counter per text), kept (the ids of the kept texts,
    ascending), out_offsets (n_kept + 1 offsets into `out`) and `out` (the kept texts, packed; None
    without a gather): int64 / int32 / uint8 device tensors from Plan.grep() -- kept, out_offsets and
    out have room for every text, their first n_kept (+ 1) entries and out_symbols symbols count --,
    numpy arrays cut to size from the host calls.  n_kept, total, need and out_symbols are Python
    ints (Plan.grep() synchronises to read them): need > capacity says that a window overflowed
    (n_kept = total = out_symbols = 0 then), out_symbols > out_capacity is the room the output needs."""

    def __init__(self, hits, kept, n_kept, total, need, out, out_offsets, out_symbols, out_capacity=None, offsets=None, n_texts=None):
        self.hits, self.kept, self.n_kept, self.total, self.need = hits, kept, n_kept, total, need
        self.out, self.out_offsets, self.out_symbols, self.out_capacity = out, out_offsets, out_symbols, out_capacity
        self.offsets, self.n_texts = offsets, n_texts      # the grep_lines calls: the n_texts + 1 offsets the buffer was cut at


def _grep_host_call(fn, what, handle, t, sym_size, off, invert, gather, out_capacity):
    """acm_gpu_grep_host / acm_grep: numpy in, a Grepped of numpy arrays out.  An output overflow is
    repeated once with the size the call reports when out_capacity is None."""
    n_texts = off.size - 1
    n_sym = int(off[-1])
    assert t.size * t.itemsize == n_sym * sym_size, "the last offset is the number of symbols"
    hits = np.zeros(n_texts, np.uint64)
    kept = np.zeros(n_texts, np.uint32)
    out_off = np.zeros(n_texts + 1, np.uint64)
    def call(cap):
        out = np.zeros(max(cap * sym_size // t.itemsize, 1), dtype=t.dtype) if gather else None
        nk, total, need = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        rc = fn(handle, _ptr(t), off.ctypes.data, n_texts, ACM_GREP_INVERT if invert else ACM_GREP_MATCHING,
                hits.ctypes.data, kept.ctypes.data, C.byref(nk), C.byref(total), _opt(out), cap if gather else 0,
                out_off.ctypes.data, C.byref(need))
        return rc, need.value, (out, nk, total)
    (out, nk, total), sym, cap = _room_call(call, what, int(out_capacity) if out_capacity is not None else n_sym, out_capacity is not None)
    k = int(nk.value)
    return Grepped(hits, kept[:k], k, int(total.value), None, out[:sym * sym_size // t.itemsize] if gather else None, out_off[:k + 1], sym, cap)


def grep_gather(text, offsets, hits, invert=False, sym_size=None, gather=True, out_capacity=None):
    """acm_grep_gather(): the kept texts of a batch under given hit counts, by the sequential pass on
    the host.  `text` (an array of symbols; with sym_size, raw bytes of symbols of that size) holds
    the texts side by side, text t = symbols [offsets[t], offsets[t + 1]).  Returns a Grepped of numpy
    arrays (hits is the argument itself; total is its sum, need None).  out_capacity (symbols; None:
    what the output needs)."""
    t = np.ascontiguousarray(text)
    sb = int(sym_size) if sym_size is not None else t.itemsize
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    h = np.ascontiguousarray(hits, dtype=np.uint64)
    n_texts = off.size - 1
    assert n_texts >= 0 and h.size == n_texts
    kept = np.zeros(max(n_texts, 1), np.uint32)
    out_off = np.zeros(n_texts + 1, np.uint64)
    nk, sym = C.c_uint64(0), C.c_uint64(0)
    flags = ACM_GREP_INVERT if invert else ACM_GREP_MATCHING

    def call(out, cap):
        return lib().acm_grep_gather(_ptr(t), sb, off.ctypes.data, n_texts, _ptr(h), flags, kept.ctypes.data, C.byref(nk), _opt(out), cap,
                                     out_off.ctypes.data, C.byref(sym))
    out = None
    if gather:
        if out_capacity is None:
            _check(call(None, 0), "acm_grep_gather")
            out_capacity = int(sym.value)
        out = np.zeros(max(int(out_capacity) * sb // t.itemsize, 1), dtype=t.dtype)
    _check(call(out, int(out_capacity) if gather else 0), "acm_grep_gather")
    k, n = int(nk.value), int(sym.value)
    return Grepped(h, kept[:k], k, int(h.sum()), None, out[:n * sb // t.itemsize] if gather else None, out_off[:k + 1], n, out_capacity)


class TalliedBatch:
    """What the tally_batch calls return: the text x keyword count matrix of a batch in CSR form.
    row_ptr (n_texts + 1 entries), col (keyword ids, ascending within a row) and val (counts): int64 /
    int32 / int64 device tensors from Plan.tally_batch() -- col and val have room for pair_capacity
    entries, their first nnz count --, uint64 / uint32 / uint64 numpy arrays cut to size from the host
    calls.  nnz, total, need and need_pairs are Python ints (Plan.tally_batch() synchronises to read
    them; the host calls leave need and need_pairs None): need > capacity says that a window
    overflowed, need_pairs > pair_capacity that the pairs did -- nnz = total = 0 then, and a repeat
    with that value has room."""

    def __init__(self, row_ptr, col, val, nnz, total, need=None, need_pairs=None):
        self.row_ptr, self.col, self.val, self.nnz, self.total, self.need, self.need_pairs = row_ptr, col, val, nnz, total, need, need_pairs

    def to_sparse_csr(self, n_keywords):
        """The matrix as a torch.sparse_csr_tensor of n_texts x n_keywords int64 counts, built on the
        arrays where they are: nothing is copied when they are device tensors."""
        import torch

        def tensor(a, dtype):
            return a.view(dtype) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).view(dtype)
        return torch.sparse_csr_tensor(tensor(self.row_ptr, torch.int64), tensor(self.col, torch.int32)[:self.nnz],
                                       tensor(self.val, torch.int64)[:self.nnz], size=(self.row_ptr.shape[0] - 1, int(n_keywords)))


def _tally_batch_host_call(fn, what, handle, t, sym_size, off):
    """acm_gpu_tally_batch_host / acm_tally_batch: numpy in, a TalliedBatch of numpy arrays out.  An
    output overflow is repeated once with the size the call reports."""
    n_texts = off.size - 1
    n_sym = int(off[-1])
    assert t.size * t.itemsize == n_sym * sym_size, "the last offset is the number of symbols"
    row_ptr = np.zeros(n_texts + 1, np.uint64)
    def call(cap):
        col, val = np.zeros(cap, np.uint32), np.zeros(cap, np.uint64)
        nnz, total = C.c_uint64(0), C.c_uint64(0)
        rc = fn(handle, _ptr(t), off.ctypes.data, n_texts, row_ptr.ctypes.data, col.ctypes.data, val.ctypes.data, cap, C.byref(nnz), C.byref(total))
        return rc, nnz.value, (col, val, total)
    (col, val, total), k, _ = _room_call(call, what, max(1024, n_sym // 16))
    return TalliedBatch(row_ptr, col[:k], val[:k], k, int(total.value))


def tally_batch_records(records, first, n_keywords):
    """acm_tally_batch_records(): the text x keyword count matrix of a batch scan's records (a
    RECORD_DTYPE array) and first[] (n_texts + 1 entries), by the sequential pass on the host.
    Returns a TalliedBatch of numpy arrays."""
    rec = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
    f = np.ascontiguousarray(first, dtype=np.uint64)
    assert f.size >= 1, "first has n_texts + 1 entries"
    n_texts = f.size - 1
    row_ptr = np.zeros(n_texts + 1, np.uint64)
    nnz = C.c_uint64(0)
    data = rec.ctypes.data if rec.size else None
    _check(lib().acm_tally_batch_records(data, f.ctypes.data, n_texts, int(n_keywords), row_ptr.ctypes.data, None, None, 0, C.byref(nnz)),
           "acm_tally_batch_records")
    k = int(nnz.value)
    col, val = np.zeros(max(k, 1), np.uint32), np.zeros(max(k, 1), np.uint64)
    _check(lib().acm_tally_batch_records(data, f.ctypes.data, n_texts, int(n_keywords), row_ptr.ctypes.data, col.ctypes.data, val.ctypes.data, k,
                                         C.byref(nnz)), "acm_tally_batch_records")
    return TalliedBatch(row_ptr, col[:k], val[:k], k, int(val[:k].sum()))


def present(k, at_least=1):
    """the term `keyword k occurs at_least times or more`"""
    return (int(k), int(at_least), ACM_RULE_NO_MAX)


def absent(k):
    """the term `keyword k does not occur`"""
    return (int(k), 0, 0)


def between(k, lo, hi):
    """the term `keyword k occurs lo to hi times` (hi = ACM_RULE_NO_MAX: no upper bound)"""
    return (int(k), int(lo), int(hi))


def rule(terms, need=None):
    """a rule: (terms, need) -- it fires when `need` of its terms (keyword_id, lo, hi) hold or more;
    need None: all of them (AND), 1: any (OR)"""
    terms = [tuple(int(x) for x in t) for t in terms]
    return terms, len(terms) if need is None else int(need)


class RuleSet:
    """rules (what rule() returns, or (terms, need) pairs) packed to the three arrays the C calls
    take: terms (uint32 [n_terms, 3]), rule_ptr (uint64, n_rules + 1) and need (uint32)."""

    def __init__(self, rules):
        rules = [r if isinstance(r[1], int) else rule(r) for r in rules]
        self.n_rules = len(rules)
        flat = [t for terms, _ in rules for t in terms]
        self.terms = np.array(flat, dtype=np.uint32).reshape(-1, 3) if flat else np.zeros((0, 3), np.uint32)
        self.rule_ptr = np.zeros(self.n_rules + 1, np.uint64)
        if rules:
            np.cumsum([len(terms) for terms, _ in rules], out=self.rule_ptr[1:])
        self.need = np.array([need for _, need in rules], dtype=np.uint32)

    def args(self):
        """(terms, rule_ptr, need, n_rules) as the C calls take them"""
        return (self.terms.ctypes.data if self.terms.size else None, self.rule_ptr.ctypes.data, self.need.ctypes.data if self.need.size else None,
                self.n_rules)

    def check(self, n_keywords):
        """acm_rules_check(): raises ACMError (ACM_GPU_E_ARG) for a set the calls would refuse"""
        _check(lib().acm_rules_check(*self.args(), int(n_keywords)), "acm_rules_check")


def _ruleset(rules):
    return rules if isinstance(rules, RuleSet) else RuleSet(rules)


class Fired:
    """What the rules calls return: the text x rule boolean matrix of a batch in CSR form.  fired_ptr
    (n_texts + 1 entries) and fired (rule ids, ascending within a row): int64 / int32 device tensors
    from Plan.rules() and Plan.rules_matrix() -- fired has room for fired_capacity entries, its first
    n_fired count --, uint64 / uint32 numpy arrays cut to size from the host calls.  n_fired, total,
    need and need_pairs are Python ints (the device calls synchronise to read them; total, need and
    need_pairs are None where no text was scanned): n_fired > fired_capacity says that `fired` had no
    room, need > capacity or need_pairs > pair_capacity that the tally in front overflowed --
    n_fired = 0 then."""

    def __init__(self, fired_ptr, fired, n_fired, total=None, need=None, need_pairs=None, fired_capacity=None):
        self.fired_ptr, self.fired, self.n_fired, self.total, self.need, self.need_pairs = fired_ptr, fired, n_fired, total, need, need_pairs
        self.fired_capacity = fired_capacity

    def to_sparse_csr(self, n_rules):
        """The matrix as a torch.sparse_csr_tensor of n_texts x n_rules ones (int8), built on the index
        arrays where they are."""
        import torch

        def tensor(a, dtype):
            return a.view(dtype) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).view(dtype)
        col = tensor(self.fired, torch.int32)[:self.n_fired]
        return torch.sparse_csr_tensor(tensor(self.fired_ptr, torch.int64), col, torch.ones(self.n_fired, dtype=torch.int8, device=col.device),
                                       size=(self.fired_ptr.shape[0] - 1, int(n_rules)))

    def rule_hits(self, n_rules):
        """in how many texts every rule fired: a bincount of `fired`"""
        import torch
        if isinstance(self.fired, torch.Tensor):
            return torch.bincount(self.fired[:self.n_fired].to(torch.int64), minlength=int(n_rules))
        return np.bincount(np.asarray(self.fired[:self.n_fired]).astype(np.int64), minlength=int(n_rules))


def _fired_host_call(call, what, n_texts, total=None):
    """call(fired_ptr, fired, capacity, n_fired) -> rc, for acm_rules_matrix / acm_gpu_rules_host /
    acm_rules: a Fired of numpy arrays out.  An output overflow is repeated once with the size the
    call reports."""
    fired_ptr = np.zeros(n_texts + 1, np.uint64)
    def room(cap):
        fired = np.zeros(cap, np.uint32)
        n = C.c_uint64(0)
        return call(fired_ptr.ctypes.data, fired.ctypes.data, cap, C.byref(n)), n.value, fired
    fired, k, cap = _room_call(room, what, max(1024, n_texts))
    return Fired(fired_ptr, fired[:k], k, int(total.value) if total is not None else None, fired_capacity=cap)


def rules_matrix(tallied, ruleset, n_keywords):
    """acm_rules_matrix(): which rules fire in which text, given the count matrix `tallied` (a
    TalliedBatch of numpy arrays), by the sequential evaluation on the host.  Returns a Fired of numpy
    arrays."""
    rs = _ruleset(ruleset)
    row_ptr = np.ascontiguousarray(tallied.row_ptr, dtype=np.uint64)
    col = np.ascontiguousarray(tallied.col, dtype=np.uint32)
    val = np.ascontiguousarray(tallied.val, dtype=np.uint64)
    assert row_ptr.size >= 1, "row_ptr has n_texts + 1 entries"

    def call(fired_ptr, fired, cap, n):
        return lib().acm_rules_matrix(row_ptr.ctypes.data, col.ctypes.data if col.size else None, val.ctypes.data if val.size else None,
                                      row_ptr.size - 1, int(n_keywords), *rs.args(), fired_ptr, fired, cap, n)
    return _fired_host_call(call, "acm_rules_matrix", row_ptr.size - 1)


def _rules_host_call(fn, what, handle, t, sym_size, off, ruleset):
    """acm_gpu_rules_host / acm_rules: numpy in, a Fired of numpy arrays out"""
    rs = _ruleset(ruleset)
    n_texts = off.size - 1
    assert t.size * t.itemsize == int(off[-1]) * sym_size, "the last offset is the number of symbols"
    total = C.c_uint64(0)

    def call(fired_ptr, fired, cap, n):
        return fn(handle, t.ctypes.data if t.size else None, off.ctypes.data, n_texts, *rs.args(), fired_ptr, fired, cap, n, C.byref(total))
    return _fired_host_call(call, what, n_texts, total)


class Indexed:
    """What the index calls return: the inverted index of a batch, the count matrix transposed, in CSR
    form over keywords -- post_ptr (n_keywords + 1 entries), post_text (text_base + t, strictly
    ascending within a keyword) and post_count.  int64 / int32 / int64 device tensors from Plan.index(),
    Plan.index_matrix() and Plan.index_concat() -- post_text and post_count have room for post_capacity
    entries, their first nnz count --, uint64 / uint32 / uint64 numpy arrays cut to size from the host
    calls.  nnz, total, need and need_pairs are Python ints as a TalliedBatch has them (total None where
    no text was scanned); forms is (lists put in order by the fast form, by the wide form) from the
    device calls, None elsewhere."""

    def __init__(self, post_ptr, post_text, post_count, nnz, total=None, text_base=0, need=None, need_pairs=None, post_capacity=None, forms=None):
        self.post_ptr, self.post_text, self.post_count, self.nnz, self.total, self.text_base = post_ptr, post_text, post_count, nnz, total, text_base
        self.need, self.need_pairs, self.post_capacity, self.forms = need, need_pairs, post_capacity, forms

    @property
    def n_keywords(self):
        return int(self.post_ptr.shape[0]) - 1

    def df(self):
        """the document frequency of every keyword, df[k] = post_ptr[k + 1] - post_ptr[k], where the index lies"""
        return self.post_ptr[1:] - self.post_ptr[:-1]

    def postings(self, k):
        """(post_text, post_count) of keyword k: views of its list"""
        a, b = int(self.post_ptr[int(k)]), int(self.post_ptr[int(k) + 1])
        return self.post_text[a:b], self.post_count[a:b]

    def to_sparse_csr(self, n_texts):
        """The index as a torch.sparse_csr_tensor of n_keywords x n_texts int64 counts (column t is text
        text_base + t), built on the arrays where they are; only the text ids are rebased when
        text_base is not 0."""
        import torch

        def tensor(a, dtype):
            return a.view(dtype) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).view(dtype)
        col = tensor(self.post_text, torch.int32)[:self.nnz]
        if self.text_base:
            col = (col.to(torch.int64) & 0xFFFFFFFF).sub_(int(self.text_base)).to(torch.int32)
        return torch.sparse_csr_tensor(tensor(self.post_ptr, torch.int64), col, tensor(self.post_count, torch.int64)[:self.nnz],
                                       size=(self.n_keywords, int(n_texts)))


def _indexed_host_call(call, what, n_keywords, text_base=0, total=None):
    """call(post_ptr, post_text, post_count, capacity, nnz) -> rc, for the host calls: an Indexed of numpy arrays
    out.  An output overflow is repeated once with the size the call reports."""
    post_ptr = np.zeros(int(n_keywords) + 1, np.uint64)
    def room(cap):
        post_text, post_count = np.zeros(cap, np.uint32), np.zeros(cap, np.uint64)
        n = C.c_uint64(0)
        return call(post_ptr.ctypes.data, post_text.ctypes.data, post_count.ctypes.data, cap, C.byref(n)), n.value, (post_text, post_count)
    (post_text, post_count), m, cap = _room_call(room, what, 1024)
    return Indexed(post_ptr, post_text[:m], post_count[:m], m, int(total.value) if total is not None else None, int(text_base), post_capacity=cap)


def index_matrix(tallied, n_keywords, text_base=0):
    """acm_index_matrix(): the inverted index of the count matrix `tallied` (a TalliedBatch of numpy
    arrays) over n_keywords keywords, by the sequential transposition on the host.  Returns an Indexed
    of numpy arrays (total: the sum of the counts)."""
    row_ptr = np.ascontiguousarray(tallied.row_ptr, dtype=np.uint64)
    col = np.ascontiguousarray(tallied.col, dtype=np.uint32)
    val = np.ascontiguousarray(tallied.val, dtype=np.uint64)
    assert row_ptr.size >= 1, "row_ptr has n_texts + 1 entries"

    def call(post_ptr, post_text, post_count, cap, n):
        return lib().acm_index_matrix(row_ptr.ctypes.data, _ptr(col), _ptr(val), row_ptr.size - 1, int(n_keywords), int(text_base), post_ptr, post_text,
                                      post_count, cap, n)
    got = _indexed_host_call(call, "acm_index_matrix", n_keywords, text_base)
    got.total = int(got.post_count.sum())
    return got


def index_concat(a, b):
    """acm_index_concat(): per keyword a's list, then b's (two Indexed of numpy arrays; a has no more
    keywords than b, and b's text ids lie above a's in every list).  Returns an Indexed of numpy arrays."""
    arrays = []
    for x in (a, b):
        arrays.append((np.ascontiguousarray(x.post_ptr, dtype=np.uint64), np.ascontiguousarray(x.post_text, dtype=np.uint32),
                       np.ascontiguousarray(x.post_count, dtype=np.uint64)))
    (ap, at, ac), (bp, bt, bc) = arrays
    assert ap.size >= 1 and bp.size >= 1, "post_ptr has n_keywords + 1 entries"

    def call(out_ptr, out_text, out_count, cap, n):
        return lib().acm_index_concat(ap.ctypes.data, _ptr(at), _ptr(ac), ap.size - 1, bp.ctypes.data, _ptr(bt), _ptr(bc), bp.size - 1, out_ptr, out_text,
                                      out_count, cap, n)
    got = _indexed_host_call(call, "acm_index_concat", bp.size - 1, a.text_base)
    got.total = a.total + b.total if a.total is not None and b.total is not None else None
    return got


def _index_host_call(fn, what, handle, t, sym_size, off, n_keywords, text_base):
    """acm_gpu_index_host / acm_index: numpy in, an Indexed of numpy arrays out"""
    n_texts = off.size - 1
    assert t.size * t.itemsize == int(off[-1]) * sym_size, "the last offset is the number of symbols"
    total = C.c_uint64(0)

    def call(post_ptr, post_text, post_count, cap, n):
        return fn(handle, t.ctypes.data if t.size else None, off.ctypes.data, n_texts, int(text_base), post_ptr, int(n_keywords), post_text, post_count,
                  cap, n, C.byref(total))
    return _indexed_host_call(call, what, n_keywords, text_base, total)


class Cooccurred:
    """What the cooccur calls return: the keyword co-occurrence matrix of a batch, the upper triangle of
    X in CSR form over keywords -- co_ptr (n_keywords + 1 entries), co_col (the ids b, strictly ascending
    within a row, b > a, or b >= a with ACM_COOCCUR_DIAGONAL) and co_val (X[a][b]).  int64 / int32 /
    int64 device tensors from Plan.cooccur(), Plan.cooccur_matrix() and Plan.cooccur_add() -- co_col and
    co_val have room for out_capacity entries, their first nnz count --, uint64 / uint32 / uint64 numpy
    arrays cut to size from the host calls.  nnz, cross (the pair instances), skipped (the texts above
    row_limit), flags, row_limit and total (the sum of the tally's counts; None where no text was
    scanned) are Python ints; need and need_pairs as a TalliedBatch has them."""

    def __init__(self, co_ptr, co_col, co_val, nnz, cross=None, skipped=None, flags=0, total=None, row_limit=0, need=None, need_pairs=None,
                 out_capacity=None):
        self.co_ptr, self.co_col, self.co_val, self.nnz, self.cross, self.skipped = co_ptr, co_col, co_val, nnz, cross, skipped
        self.flags, self.total, self.row_limit, self.need, self.need_pairs, self.out_capacity = flags, total, row_limit, need, need_pairs, out_capacity

    @property
    def n_keywords(self):
        return int(self.co_ptr.shape[0]) - 1

    def row(self, a):
        """(ids, values) of row a: views of its entries, the keywords b that occur with a and X[a][b]"""
        lo, hi = int(self.co_ptr[int(a)]), int(self.co_ptr[int(a) + 1])
        return self.co_col[lo:hi], self.co_val[lo:hi]

    def value(self, a, b):
        """X[a][b] as a Python int, the ids in either order; 0 where the matrix has no entry"""
        a, b = min(int(a), int(b)), max(int(a), int(b))
        ids, values = self.row(a)
        hit = (ids == b).nonzero()
        hit = hit[0] if isinstance(hit, tuple) else hit.reshape(-1)
        return int(values[int(hit[0])]) & 0xFFFFFFFFFFFFFFFF if len(hit) else 0

    def to_sparse_csr(self, n_keywords=None):
        """The upper triangle as a torch.sparse_csr_tensor of n_keywords x n_keywords int64 values, built
        on the arrays where they are: nothing is copied when they are device tensors."""
        import torch

        def tensor(a, dtype):
            return a.view(dtype) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).view(dtype)
        nk = self.n_keywords if n_keywords is None else int(n_keywords)
        assert nk == self.n_keywords, "co_ptr has n_keywords + 1 entries"
        return torch.sparse_csr_tensor(tensor(self.co_ptr, torch.int64), tensor(self.co_col, torch.int32)[:self.nnz],
                                       tensor(self.co_val, torch.int64)[:self.nnz], size=(nk, nk))


def _cooccur_flags(flags):
    flags = int(flags)
    if flags & ~(ACM_COOCCUR_PRODUCT | ACM_COOCCUR_DIAGONAL):
        raise ACMError(ACM_GPU_E_ARG, "cooccur: flags is a bit set of ACM_COOCCUR_PRODUCT and ACM_COOCCUR_DIAGONAL")
    return flags


def _cooccurred_host_call(call, what, n_keywords, flags=0, row_limit=0, total=None):
    """call(co_ptr, co_col, co_val, capacity, nnz, cross, skipped) -> rc, for the host calls: a Cooccurred of numpy
    arrays out.  An output overflow is repeated once with the size the call reports."""
    co_ptr = np.zeros(int(n_keywords) + 1, np.uint64)
    cross, skipped = C.c_uint64(0), C.c_uint64(0)
    def room(cap):
        co_col, co_val = np.zeros(cap, np.uint32), np.zeros(cap, np.uint64)
        n = C.c_uint64(0)
        return call(co_ptr.ctypes.data, co_col.ctypes.data, co_val.ctypes.data, cap, C.byref(n), C.byref(cross), C.byref(skipped)), n.value, (co_col, co_val)
    (co_col, co_val), m, cap = _room_call(room, what, 1024)
    return Cooccurred(co_ptr, co_col[:m], co_val[:m], m, int(cross.value), int(skipped.value), int(flags),
                      int(total.value) if total is not None else None, int(row_limit), out_capacity=cap)


def cooccur_matrix(tallied, flags=0, row_limit=0, n_keywords=None):
    """acm_cooccur_matrix(): the co-occurrence matrix of the count matrix `tallied` (a TalliedBatch of
    numpy arrays) over n_keywords keywords (None: one more than the greatest id it holds), by the
    sequential definition on the host.  Returns a Cooccurred of numpy arrays."""
    row_ptr = np.ascontiguousarray(tallied.row_ptr, dtype=np.uint64)
    col = np.ascontiguousarray(tallied.col, dtype=np.uint32)
    val = np.ascontiguousarray(tallied.val, dtype=np.uint64)
    assert row_ptr.size >= 1, "row_ptr has n_texts + 1 entries"
    nk = int(n_keywords) if n_keywords is not None else (int(col.max()) + 1 if col.size else 0)

    def call(co_ptr, co_col, co_val, cap, n, cross, skipped):
        return lib().acm_cooccur_matrix(row_ptr.ctypes.data, _ptr(col), _ptr(val), row_ptr.size - 1, nk, int(flags), int(row_limit), co_ptr, co_col,
                                        co_val, cap, n, cross, skipped)
    return _cooccurred_host_call(call, "acm_cooccur_matrix", nk, flags, row_limit)


def _sum_or_none(x, y):
    return x + y if x is not None and y is not None else None


def cooccur_add(a, b):
    """acm_cooccur_add(): the entrywise sum of two Cooccurred of numpy arrays (a has no more keywords than
    b; both under the same flags and row_limit).  Returns a Cooccurred of numpy arrays; cross, skipped and
    total are the sums."""
    arrays = []
    for x in (a, b):
        arrays.append((np.ascontiguousarray(x.co_ptr, dtype=np.uint64), np.ascontiguousarray(x.co_col, dtype=np.uint32),
                       np.ascontiguousarray(x.co_val, dtype=np.uint64)))
    (ap, ac, av), (bp, bc, bv) = arrays
    assert ap.size >= 1 and bp.size >= 1, "co_ptr has n_keywords + 1 entries"

    def call(out_ptr, out_col, out_val, cap, n, cross, skipped):
        return lib().acm_cooccur_add(ap.ctypes.data, _ptr(ac), _ptr(av), ap.size - 1, bp.ctypes.data, _ptr(bc), _ptr(bv), bp.size - 1, out_ptr, out_col,
                                     out_val, cap, n)
    got = _cooccurred_host_call(call, "acm_cooccur_add", bp.size - 1, b.flags, b.row_limit)
    got.cross, got.skipped, got.total = _sum_or_none(a.cross, b.cross), _sum_or_none(a.skipped, b.skipped), _sum_or_none(a.total, b.total)
    return got


def _cooccur_host_call(fn, what, handle, t, sym_size, off, n_keywords, flags, row_limit):
    """acm_gpu_cooccur_host / acm_cooccur: numpy in, a Cooccurred of numpy arrays out"""
    n_texts = off.size - 1
    assert t.size * t.itemsize == int(off[-1]) * sym_size, "the last offset is the number of symbols"
    total = C.c_uint64(0)

    def call(co_ptr, co_col, co_val, cap, n, cross, skipped):
        return fn(handle, t.ctypes.data if t.size else None, off.ctypes.data, n_texts, int(n_keywords), int(flags), int(row_limit), co_ptr, co_col,
                  co_val, cap, n, cross, skipped, C.byref(total))
    return _cooccurred_host_call(call, what, n_keywords, flags, row_limit, total)


def weight(k, w, cap=None):
    """the term `w times the count of keyword k`, the count taken as at most `cap` (None: no cap; 1: presence)"""
    return (int(k), int(w), ACM_SCORE_NO_CAP if cap is None else int(cap))


def score_class(terms, bias=0, threshold=1):
    """a class: (terms, bias, threshold) -- its score is bias + the sum of its weight() terms, kept where it reaches threshold"""
    return [tuple(int(x) for x in t) for t in terms], int(bias), int(threshold)


SCORE_TERM_DTYPE = np.dtype([("keyword_id", "<u4"), ("weight", "<i4"), ("cap", "<u4")])


class ScoreModel:
    """classes (what score_class() returns) packed to the four arrays the C calls take: terms
    (SCORE_TERM_DTYPE), class_ptr (uint64, n_classes + 1), bias and threshold (int64)."""

    def __init__(self, classes):
        classes = [c if len(c) == 3 and isinstance(c[1], int) else score_class(c) for c in classes]
        self.n_classes = len(classes)
        flat = [t for terms, _, _ in classes for t in terms]
        self.terms = np.array(flat, dtype=SCORE_TERM_DTYPE) if flat else np.zeros(0, SCORE_TERM_DTYPE)
        self.class_ptr = np.zeros(self.n_classes + 1, np.uint64)
        if classes:
            np.cumsum([len(terms) for terms, _, _ in classes], out=self.class_ptr[1:])
        self.bias = np.array([b for _, b, _ in classes], dtype=np.int64)
        self.threshold = np.array([t for _, _, t in classes], dtype=np.int64)

    def args(self):
        """(terms, class_ptr, bias, threshold, n_classes) as the C calls take them"""
        return (self.terms.ctypes.data if self.terms.size else None, self.class_ptr.ctypes.data, self.bias.ctypes.data if self.n_classes else None,
                self.threshold.ctypes.data if self.n_classes else None, self.n_classes)

    def check(self, n_keywords):
        """acm_score_check(): raises ACMError (ACM_GPU_E_ARG) for a model the calls would refuse"""
        _check(lib().acm_score_check(*self.args(), int(n_keywords)), "acm_score_check")


def _scoremodel(model):
    return model if isinstance(model, ScoreModel) else ScoreModel(model)


class Scored:
    """What the score calls return: the kept part of the text x class score matrix of a batch in CSR
    form -- kept_ptr (n_texts + 1 entries), kept_class (ascending within a row) and kept_score --, best
    (the class of every text's largest kept score, ACM_SCORE_NONE for an empty row; None where the call
    did not make it) and, from a call with k > 0, class_hits (kept texts per class), top_n, top_text and
    top_score ([n_classes, k]; ACM_SCORE_NONE and 0 beyond top_n).  int64 / int32 device tensors from
    Plan.score(), Plan.score_matrix() and Plan.score_top() -- the kept arrays have room for kept_capacity
    entries, their first n_kept count --, numpy arrays cut to size from the host calls.  n_kept, total,
    need and need_pairs are Python ints as Fired has them: n_kept > kept_capacity says that the kept
    arrays had no room (best is unspecified, the top arrays are zero then), need > capacity or
    need_pairs > pair_capacity that the tally in front overflowed -- n_kept = 0 then."""

    def __init__(self, kept_ptr, kept_class, kept_score, n_kept, best=None, class_hits=None, top_n=None, top_text=None, top_score=None, total=None,
                 need=None, need_pairs=None, kept_capacity=None):
        self.kept_ptr, self.kept_class, self.kept_score, self.n_kept, self.best = kept_ptr, kept_class, kept_score, n_kept, best
        self.class_hits, self.top_n, self.top_text, self.top_score = class_hits, top_n, top_text, top_score
        self.total, self.need, self.need_pairs, self.kept_capacity = total, need, need_pairs, kept_capacity

    def to_sparse_csr(self, n_classes):
        """The kept scores as a torch.sparse_csr_tensor of n_texts x n_classes (int64), built on the
        arrays where they are."""
        import torch

        def tensor(a, dtype):
            return a.view(dtype) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).view(dtype)
        return torch.sparse_csr_tensor(tensor(self.kept_ptr, torch.int64), tensor(self.kept_class, torch.int32)[:self.n_kept],
                                       tensor(self.kept_score, torch.int64)[:self.n_kept], size=(self.kept_ptr.shape[0] - 1, int(n_classes)))


def _top_host_arrays(n_classes, k):
    return (np.zeros(n_classes, np.uint64), np.zeros(n_classes, np.uint32), np.zeros((n_classes, k), np.uint32), np.zeros((n_classes, k), np.int64))


def _scored_host_call(call, what, n_texts, n_classes, k, total=None):
    """call(kept_ptr, kept_class, kept_score, capacity, n_kept, best, top arrays...) -> rc, for acm_score_matrix /
    acm_gpu_score_host / acm_score: a Scored of numpy arrays out.  An output overflow is repeated once with the size
    the call reports."""
    kept_ptr, best = np.zeros(n_texts + 1, np.uint64), np.full(n_texts, ACM_SCORE_NONE, np.uint32)
    hits, top_n, top_text, top_score = _top_host_arrays(n_classes, k)
    def room(cap):
        kept_class, kept_score = np.zeros(cap, np.uint32), np.zeros(cap, np.int64)
        n = C.c_uint64(0)
        rc = call(kept_ptr.ctypes.data, kept_class.ctypes.data, kept_score.ctypes.data, cap, C.byref(n), _ptr(best), _ptr(hits), _ptr(top_n),
                  _ptr(top_text), _ptr(top_score))
        return rc, n.value, (kept_class, kept_score)
    (kept_class, kept_score), m, cap = _room_call(room, what, max(1024, n_texts))
    top = (hits, top_n, top_text, top_score) if k else (None, None, None, None)
    return Scored(kept_ptr, kept_class[:m], kept_score[:m], m, best, *top, total=int(total.value) if total is not None else None, kept_capacity=cap)


def score_matrix(tallied, model, n_keywords):
    """acm_score_matrix(): the kept scores of every text, given the count matrix `tallied` (a
    TalliedBatch of numpy arrays), by the sequential evaluation on the host.  Returns a Scored of numpy
    arrays (no top arrays: score_top())."""
    sm = _scoremodel(model)
    row_ptr = np.ascontiguousarray(tallied.row_ptr, dtype=np.uint64)
    col = np.ascontiguousarray(tallied.col, dtype=np.uint32)
    val = np.ascontiguousarray(tallied.val, dtype=np.uint64)
    assert row_ptr.size >= 1, "row_ptr has n_texts + 1 entries"

    def call(kept_ptr, kept_class, kept_score, cap, n, best, *top):
        return lib().acm_score_matrix(row_ptr.ctypes.data, _ptr(col), _ptr(val), row_ptr.size - 1, int(n_keywords), *sm.args(), kept_ptr, kept_class,
                                      kept_score, cap, n, best)
    return _scored_host_call(call, "acm_score_matrix", row_ptr.size - 1, sm.n_classes, 0)


def score_top(scored, n_classes, k):
    """acm_score_top(): TOP of a Scored of numpy arrays on the host; returns it with class_hits, top_n, top_text and
    top_score ([n_classes, k]) filled in."""
    kept_ptr = np.ascontiguousarray(scored.kept_ptr, dtype=np.uint64)
    kept_class = np.ascontiguousarray(scored.kept_class, dtype=np.uint32)
    kept_score = np.ascontiguousarray(scored.kept_score, dtype=np.int64)
    hits, top_n, top_text, top_score = _top_host_arrays(int(n_classes), int(k))
    _check(lib().acm_score_top(kept_ptr.ctypes.data, _ptr(kept_class), _ptr(kept_score), kept_ptr.size - 1, int(n_classes), int(k), _ptr(hits),
                               _ptr(top_n), _ptr(top_text), _ptr(top_score)), "acm_score_top")
    scored.class_hits, scored.top_n, scored.top_text, scored.top_score = hits, top_n, top_text, top_score
    return scored


def _score_host_call(fn, what, handle, t, sym_size, off, model, k):
    """acm_gpu_score_host / acm_score: numpy in, a Scored of numpy arrays out"""
    sm = _scoremodel(model)
    n_texts = off.size - 1
    assert t.size * t.itemsize == int(off[-1]) * sym_size, "the last offset is the number of symbols"
    total = C.c_uint64(0)

    def call(kept_ptr, kept_class, kept_score, cap, n, best, hits, top_n, top_text, top_score):
        return fn(handle, t.ctypes.data if t.size else None, off.ctypes.data, n_texts, *sm.args(), kept_ptr, kept_class, kept_score, cap, n, best,
                  int(k), hits, top_n, top_text, top_score, C.byref(total))
    return _scored_host_call(call, what, n_texts, sm.n_classes, int(k), total)


class PatternSet:
    """Patterns with don't-care gaps packed to the two arrays the C calls take: terms (uint32 [n_terms, 3]:
    keyword_id, offset, length) and pat_ptr (uint64, n_patterns + 1).  `patterns`: one list of (keyword_id,
    offset, length) terms per pattern -- keyword keyword_id, `length` symbols long, begins `offset` symbols
    behind the pattern's first symbol.  from_templates() makes one from templates with a wildcard symbol."""

    def __init__(self, patterns):
        patterns = [list(p) for p in patterns]
        self.n_patterns = len(patterns)
        flat = [tuple(int(x) for x in t) for p in patterns for t in p]
        self.terms = np.array(flat, dtype=np.uint32).reshape(-1, 3)
        self.pat_ptr = np.zeros(self.n_patterns + 1, np.uint64)
        if patterns:
            np.cumsum([len(p) for p in patterns], out=self.pat_ptr[1:])
        self.n_keywords = int(self.terms[:, 0].max()) + 1 if self.terms.size else 0   # what the host pass is told when nothing else is known

    @classmethod
    def from_templates(cls, machine, templates, wildcard=None):
        """A template is a sequence of symbols (bytes, or an array of symbol values) in which `wildcard` (a
        symbol value; for bytes also a 1-byte string) marks a don't-care that matches any one symbol.  Every
        template is cut into its maximal don't-care-free runs; the runs `machine` does not hold yet are
        inserted, those it holds keep their ids.  ValueError for a template that ends in a don't-care or has
        no symbol.  Returns the PatternSet (n_keywords = the machine's keywords afterwards)."""
        if isinstance(wildcard, (bytes, bytearray)):
            wildcard = wildcard[0]
        known = None
        patterns = []
        for tpl in templates:
            sym = [int(x) for x in (bytes(tpl) if isinstance(tpl, (bytes, bytearray)) else np.asarray(tpl).reshape(-1))]
            if not sym or all(x == wildcard for x in sym):
                raise ValueError("a template needs a symbol that is no don't-care")
            if wildcard is not None and sym[-1] == wildcard:
                raise ValueError("a template cannot end in a don't-care: it would test nothing but that the text goes on")
            terms, i = [], 0
            while i < len(sym):
                if wildcard is not None and sym[i] == wildcard:
                    i += 1
                    continue
                j = i
                while j < len(sym) and (wildcard is None or sym[j] != wildcard):
                    j += 1
                run = np.array(sym[i:j], dtype=_SYM_DTYPE[machine.sym_size])
                before = machine.nb_keywords
                machine.add_keyword(run)
                if machine.nb_keywords > before:
                    kid = before
                    if known is not None:
                        known[machine.keyword(kid)[0]] = kid
                else:                                              # held already: the dictionary's spelling of the run says which
                    if known is None:
                        known = {machine.keyword(k)[0]: k for k in range(machine.nb_keywords)}
                    spelt = [w for e, length, w, _ in machine.match_loop(run) if e == run.size - 1 and length == run.size]
                    kid = known[spelt[0]]
                terms.append((kid, i, j - i))
                i = j
            patterns.append(terms)
        ps = cls(patterns)
        ps.n_keywords = machine.nb_keywords
        return ps

    def args(self):
        """(terms, pat_ptr, n_patterns) as the C calls take them"""
        return self.terms.ctypes.data if self.terms.size else None, self.pat_ptr.ctypes.data, self.n_patterns

    def check(self, n_keywords):
        """acm_patterns_check(): raises ACMError (ACM_GPU_E_ARG) for a set the calls would refuse"""
        _check(lib().acm_patterns_check(*self.args(), int(n_keywords)), "acm_patterns_check")


def _patternset(patterns):
    return patterns if isinstance(patterns, PatternSet) else PatternSet(patterns)


def patterns_records(records, patternset, n_symbols, offsets=None, pos_base=0, n_keywords=None, out_capacity=None):
    """acm_patterns_records(): the matches of the patterns of `patternset` among `records` (RECORD_DTYPE, in
    canonical order, positions pos_base + index into a buffer of n_symbols symbols), by the sequential pass
    on the host: one record (end_pos of the match's last symbol, the pattern's length, the pattern's id) per
    match, by end_pos ascending, length descending, pattern id ascending.  `offsets` (n_texts + 1 entries)
    cuts the buffer into texts; a match lies inside one text.  out_capacity None: counted first, then sized
    by the count; given and too small: ACMError (ACM_GPU_E_OVERFLOW)."""
    return _terms_records("acm_patterns_records", records, _patternset(patternset), n_symbols, offsets, pos_base, n_keywords, out_capacity)


def _terms_records(name, records, tset, n_symbols, offsets, pos_base, n_keywords, out_capacity):
    """what patterns_records(), chains_records() and near_records() share: the C call `name` on numpy arrays, counted first when
    no capacity is given"""
    fn = getattr(lib(), name)
    a = np.ascontiguousarray(np.asarray(records, dtype=RECORD_DTYPE).reshape(-1))
    off = np.ascontiguousarray(offsets, dtype=np.uint64) if offsets is not None else None
    nk = int(n_keywords) if n_keywords is not None else tset.n_keywords
    n = C.c_uint64(0)

    def call(out, cap):
        return fn(_ptr(a), a.size, int(n_symbols), int(pos_base), *_cut(off), *tset.args(), nk, _opt(out), cap, C.byref(n))
    if out_capacity is None:                                       # (no output: the call only counts)
        _check(call(None, 0), name)
        out_capacity = int(n.value)
    out = np.zeros(max(int(out_capacity), 1), dtype=RECORD_DTYPE)
    _check(call(out, int(out_capacity)), name)
    return out[:n.value]


class ChainSet:
    """Keyword chains with bounded gaps packed to the two arrays the C calls take: terms (uint32 [n_terms, 3]:
    keyword_id, gap_min, gap_max) and chain_ptr (uint64, n_chains + 1).  `chains`: one list of (keyword_id,
    gap_min, gap_max) terms per chain, in order -- the keyword begins gap_min to gap_max symbols behind the
    last symbol of the term in front; a chain's first term has the gaps 0, 0.  from_specs() makes one from
    keywords and gaps."""

    def __init__(self, chains):
        chains = [list(c) for c in chains]
        self.n_chains = len(chains)
        flat = [tuple(int(x) for x in t) for c in chains for t in c]
        self.terms = np.array(flat, dtype=np.uint32).reshape(-1, 3)
        self.chain_ptr = np.zeros(self.n_chains + 1, np.uint64)
        if chains:
            np.cumsum([len(c) for c in chains], out=self.chain_ptr[1:])
        self.n_keywords = int(self.terms[:, 0].max()) + 1 if self.terms.size else 0   # what the host pass is told when nothing else is known

    @classmethod
    def from_specs(cls, machine, specs):
        """A spec is [kw0, (min, max), kw1, (min, max), kw2, ...]: keywords (bytes, or arrays of symbol values)
        with the bounds of the gap between each two.  The keywords `machine` does not hold yet are inserted,
        those it holds keep their ids.  ValueError for a spec of another shape.  Returns the ChainSet
        (n_keywords = the machine's keywords afterwards)."""
        known = None
        chains = []
        for spec in specs:
            spec = list(spec)
            if len(spec) % 2 == 0:
                raise ValueError("a chain is keyword, (min, max), keyword, ...: it begins and ends with a keyword")
            terms = []
            for j in range(0, len(spec), 2):
                kw = spec[j]
                run = np.frombuffer(bytes(kw), np.uint8) if isinstance(kw, (bytes, bytearray)) else np.asarray(kw).reshape(-1)
                run = run.astype(_SYM_DTYPE[machine.sym_size])
                if run.size == 0:
                    raise ValueError("a keyword needs a symbol")
                before = machine.nb_keywords
                machine.add_keyword(run)
                if machine.nb_keywords > before:
                    kid = before
                    if known is not None:
                        known[machine.keyword(kid)[0]] = kid
                else:                                              # held already: the dictionary's spelling of the run says which
                    if known is None:
                        known = {machine.keyword(k)[0]: k for k in range(machine.nb_keywords)}
                    spelt = [w for e, length, w, _ in machine.match_loop(run) if e == run.size - 1 and length == run.size]
                    kid = known[spelt[0]]
                gap = (0, 0) if j == 0 else tuple(int(x) for x in spec[j - 1])
                if len(gap) != 2:
                    raise ValueError("a gap is (min, max)")
                terms.append((kid, gap[0], gap[1]))
            chains.append(terms)
        cs = cls(chains)
        cs.n_keywords = machine.nb_keywords
        return cs

    def args(self):
        """(terms, chain_ptr, n_chains) as the C calls take them"""
        return self.terms.ctypes.data if self.terms.size else None, self.chain_ptr.ctypes.data, self.n_chains

    def check(self, n_keywords):
        """acm_chains_check(): raises ACMError (ACM_GPU_E_ARG) for a set the calls would refuse"""
        _check(lib().acm_chains_check(*self.args(), int(n_keywords)), "acm_chains_check")


def _chainset(chains):
    return chains if isinstance(chains, ChainSet) else ChainSet(chains)


def chains_records(records, chainset, n_symbols, offsets=None, pos_base=0, n_keywords=None, out_capacity=None):
    """acm_chains_records(): the matches of the chains of `chainset` among `records` (RECORD_DTYPE, in canonical
    order, positions pos_base + index into a buffer of n_symbols symbols), by the sequential pass on the
    host: per chain and end one record (end_pos of the match's last symbol, the length of the shortest match
    that ends there, the chain's id), by end_pos ascending, length descending, chain id ascending.  `offsets`
    (n_texts + 1 entries) cuts the buffer into texts; a match lies inside one text.  out_capacity None:
    counted first, then sized by the count; given and too small: ACMError (ACM_GPU_E_OVERFLOW)."""
    return _terms_records("acm_chains_records", records, _chainset(chainset), n_symbols, offsets, pos_base, n_keywords, out_capacity)


class NearSet:
    """NEAR/n groups packed to the three arrays the C calls take: terms (uint32, the keyword ids of all groups),
    group_ptr (uint64, n_groups + 1) and groups (uint32 [n_groups, 2]: width, need).  `groups`: one entry per
    group, a list of keyword ids -- it takes the `width=` and `need=` given here -- or (ids, width) or (ids,
    width, need).  A group matches where at least `need` of its keywords (0: all of them) occur, in any order
    and overlapping or not, inside `width` symbols of one text."""

    def __init__(self, groups, width=None, need=0):
        packed = []
        for g in groups:
            if isinstance(g, tuple) and len(g) in (2, 3) and not np.isscalar(g[0]):
                ids, w, k = (g + (need,))[:3]
            else:
                ids, w, k = g, width, need
            if w is None:
                raise ValueError("a group needs a width")
            packed.append(([int(x) for x in ids], int(w), int(k)))
        self.n_groups = len(packed)
        self.terms = np.array([x for ids, _, _ in packed for x in ids], dtype=np.uint32)
        self.group_ptr = np.zeros(self.n_groups + 1, np.uint64)
        if packed:
            np.cumsum([len(ids) for ids, _, _ in packed], out=self.group_ptr[1:])
        self.groups = np.array([(w, k) for _, w, k in packed], dtype=np.uint32).reshape(-1, 2)
        self.n_keywords = int(self.terms.max()) + 1 if self.terms.size else 0   # what the host pass is told when nothing else is known

    def args(self):
        """(terms, group_ptr, groups, n_groups) as the C calls take them"""
        return (self.terms.ctypes.data if self.terms.size else None, self.group_ptr.ctypes.data,
                self.groups.ctypes.data if self.groups.size else None, self.n_groups)

    def check(self, n_keywords):
        """acm_near_check(): raises ACMError (ACM_GPU_E_ARG) for a set the calls would refuse"""
        _check(lib().acm_near_check(*self.args(), int(n_keywords)), "acm_near_check")


def _nearset(groups):
    return groups if isinstance(groups, NearSet) else NearSet(groups)


def near_records(records, nearset, n_symbols, offsets=None, pos_base=0, n_keywords=None, out_capacity=None):
    """acm_near_records(): the matches of the groups of `nearset` among `records` (RECORD_DTYPE, in canonical
    order, positions pos_base + index into a buffer of n_symbols symbols), by the sequential pass on the
    host: per group and end one record (end_pos of the window's last symbol, the length of the shortest
    window that ends there, the group's id), by end_pos ascending, length descending, group id ascending.
    `offsets` (n_texts + 1 entries) cuts the buffer into texts; a window lies inside one text.  out_capacity
    None: counted first, then sized by the count; given and too small: ACMError (ACM_GPU_E_OVERFLOW)."""
    return _terms_records("acm_near_records", records, _nearset(nearset), n_symbols, offsets, pos_base, n_keywords, out_capacity)


class _PieceKeywords:
    """the pieces of targets as keywords of `machine`: add() inserts a piece the machine does not hold yet (in order of
    first appearance) and returns the id of the keyword that is the piece"""

    def __init__(self, machine):
        self.machine = machine
        self.known = None

    def add(self, piece):
        machine = self.machine
        run = np.array(piece, dtype=_SYM_DTYPE[machine.sym_size])
        before = machine.nb_keywords
        machine.add_keyword(run)
        if machine.nb_keywords > before:
            if self.known is not None:
                self.known[machine.keyword(before)[0]] = before
            return before
        if self.known is None:                                     # held already: the dictionary's spelling of the piece says which
            self.known = {machine.keyword(i)[0]: i for i in range(machine.nb_keywords)}
        spelling = [w for at, length, w, _ in machine.match_loop(run) if at == run.size - 1 and length == run.size]
        return self.known[spelling[0]]


class ApproxSet:
    """Targets with a mismatch budget packed to the arrays the C calls take: spell_data (the spellings side by
    side, symbols of `sym_size` bytes), spell_off (uint64, n_targets + 1), k (uint32 per target), terms (uint32
    [n_terms, 3]: keyword_id, offset, length) and tgt_ptr (uint64, n_targets + 1).  `targets`: one spelling per
    target (bytes, or an array of symbols); `k`: a scalar or one budget per target; `terms`: one list of
    (keyword_id, offset, length) per target -- keyword keyword_id, `length` symbols long, is the piece of the
    spelling that begins at `offset`.  from_targets() makes one by the canonical cut."""

    def __init__(self, targets, k, terms, sym_size=None):
        targets = list(targets)
        if sym_size is None:
            sym_size = next((np.asarray(t).dtype.itemsize for t in targets if not isinstance(t, (bytes, bytearray))), 1)
        self.sym_size = int(sym_size)
        dt = _SYM_DTYPE[self.sym_size]
        spelt = [np.frombuffer(bytes(t), np.uint8).astype(dt) if isinstance(t, (bytes, bytearray)) else np.ascontiguousarray(t, dtype=dt).reshape(-1)
                 for t in targets]
        self.n_targets = len(spelt)
        self.spell_data = np.ascontiguousarray(np.concatenate(spelt)) if spelt else np.zeros(0, dt)
        self.spell_off = np.zeros(self.n_targets + 1, np.uint64)
        self.k = np.ascontiguousarray(np.broadcast_to(np.asarray(k, dtype=np.uint32), (self.n_targets,)))
        terms = [list(t) for t in terms]
        assert len(terms) == self.n_targets, "one list of terms per target"
        flat = [tuple(int(x) for x in t) for p in terms for t in p]
        self.terms = np.array(flat, dtype=np.uint32).reshape(-1, 3)
        self.tgt_ptr = np.zeros(self.n_targets + 1, np.uint64)
        if spelt:
            np.cumsum([t.size for t in spelt], out=self.spell_off[1:])
            np.cumsum([len(p) for p in terms], out=self.tgt_ptr[1:])
        self.n_keywords = int(self.terms[:, 0].max()) + 1 if self.terms.size else 0   # what the host pass is told when nothing else is known

    @classmethod
    def from_targets(cls, machine, targets, k):
        """Every target is cut into k + 1 pieces by the canonical cut (acm_approx_split: piece j is [j * L // (k + 1),
        (j + 1) * L // (k + 1))); the distinct pieces `machine` does not hold yet are inserted as keywords in order
        of first appearance, those it holds keep their ids.  `k`: a scalar or one per target.  ValueError for a
        target shorter than k + 1 symbols.  Returns the ApproxSet (n_keywords = the machine's keywords afterwards)."""
        targets = list(targets)
        ks = [int(x) for x in np.broadcast_to(np.asarray(k), (len(targets),))]
        pieces = _PieceKeywords(machine)
        spelt, terms = [], []
        for tgt, kk in zip(targets, ks):
            sym = machine._symbols(tgt).reshape(-1)
            if sym.size < kk + 1:
                raise ValueError("a target of %d symbols cannot be cut into %d pieces" % (sym.size, kk + 1))
            mine = []
            for j in range(kk + 1):
                b, e = C.c_uint64(0), C.c_uint64(0)
                _check(lib().acm_approx_split(sym.size, kk, j, C.byref(b), C.byref(e)), "acm_approx_split")
                mine.append((pieces.add(sym[b.value:e.value]), int(b.value), int(e.value - b.value)))
            spelt.append(sym)
            terms.append(mine)
        aset = cls(spelt, ks, terms, sym_size=machine.sym_size)
        aset.n_keywords = machine.nb_keywords
        return aset

    def args(self):
        """(spell_data, spell_off, k, terms, tgt_ptr, n_targets) as the C calls take them"""
        return (self.spell_data.ctypes.data if self.spell_data.size else None, self.spell_off.ctypes.data, self.k.ctypes.data if self.k.size else None,
                self.terms.ctypes.data if self.terms.size else None, self.tgt_ptr.ctypes.data, self.n_targets)

    def check(self, n_keywords):
        """acm_approx_check(): raises ACMError (ACM_GPU_E_ARG) for a set the calls would refuse"""
        _check(lib().acm_approx_check(*self.args()[1:], int(n_keywords)), "acm_approx_check")

    def check_edit(self, n_keywords=None):
        """acm_edit_check(): raises ACMError (ACM_GPU_E_ARG) for a set the edit calls would refuse -- acm_approx_check's
        errors, a budget above 15, a budget that is not below its target's length"""
        _check(lib().acm_edit_check(*self.args()[1:], int(n_keywords) if n_keywords is not None else self.n_keywords), "acm_edit_check")


def approx_records(records, approxset, text, offsets=None, pos_base=0, n_keywords=None, out_capacity=None):
    """acm_approx_records(): the occurrences with at most k mismatches of the targets of `approxset` (an
    ApproxSet) that the `records` seed (RECORD_DTYPE, in canonical order, positions pos_base + index into
    `text`, an array of symbols of the set's size or bytes), by the sequential pass on the host.  Returns
    (matches, dist): one record (end_pos of the last symbol, the target's length, the target's id) per match,
    by end_pos ascending, length descending, target id ascending, and the mismatches of each.  `offsets`
    (n_texts + 1 entries) cuts the buffer into texts; a match lies inside one text.  out_capacity None: counted
    first, then sized by the count; given and too small: ACMError (ACM_GPU_E_OVERFLOW)."""
    return _set_records("acm_approx_records", records, approxset, text, offsets, pos_base, n_keywords, out_capacity)


def edit_records(records, approxset, text, offsets=None, pos_base=0, n_keywords=None, out_capacity=None):
    """acm_edit_records(): the ends at which the targets of `approxset` (an ApproxSet; check_edit() says whether the
    edit calls take it) occur within edit distance k among those the `records` seed, by the sequential pass on the
    host; arguments and order as approx_records().  Returns (matches, dist): one record (end_pos of the last
    symbol, the length of the shortest best match ending there, the target's id) per (target, end), and the edit
    distance of each."""
    return _set_records("acm_edit_records", records, approxset, text, offsets, pos_base, n_keywords, out_capacity)


def _set_records(name, records, aset, text, offsets, pos_base, n_keywords, out_capacity):
    """what approx_records() and edit_records() share: the C call `name` on numpy arrays, counted first when no
    capacity is given"""
    fn = getattr(lib(), name)
    a = np.ascontiguousarray(np.asarray(records, dtype=RECORD_DTYPE).reshape(-1))
    t = np.frombuffer(bytes(text), np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text)
    n_symbols = t.size * t.itemsize // aset.sym_size
    off = np.ascontiguousarray(offsets, dtype=np.uint64) if offsets is not None else None
    nk = int(n_keywords) if n_keywords is not None else aset.n_keywords
    n = C.c_uint64(0)

    def call(out, dist, cap):
        return fn(_ptr(a), a.size, _ptr(t), aset.sym_size, n_symbols, int(pos_base), *_cut(off), *aset.args(), nk, _opt(out), _opt(dist), cap, C.byref(n))
    if out_capacity is None:                                       # (no output: the call only counts)
        _check(call(None, None, 0), name)
        out_capacity = int(n.value)
    out = np.zeros(max(int(out_capacity), 1), dtype=RECORD_DTYPE)
    dist = np.zeros(max(int(out_capacity), 1), dtype=np.uint32)
    _check(call(out, dist, int(out_capacity)), name)
    return out[:n.value], dist[:n.value]


ACM_TEMPLATE_LITERAL = 0xFFFFFFFF
ACM_TEMPLATE_ANY = 0xFFFFFFFE
ACM_TEMPLATE_NEGATED = 1
ACM_TEMPLATE_MAX_RANGES = 16


class _Any:
    """the cell that accepts every symbol"""

    def __repr__(self):
        return "ANY"


ANY = _Any()


class SymbolClass:
    """A cell that accepts a set of symbols: `ranges` holds symbols and inclusive (lo, hi) pairs, at most 16 in all;
    with `negate` the cell accepts every symbol outside them.  Equal classes compare equal and share an id in a
    TemplateSet."""

    def __init__(self, ranges, negate=False):
        self.ranges = tuple((int(r), int(r)) if np.isscalar(r) else (int(r[0]), int(r[1])) for r in ranges)
        self.negate = bool(negate)

    def _key(self):
        return (self.ranges, self.negate)

    def __eq__(self, other):
        return isinstance(other, SymbolClass) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "SymbolClass(%r%s)" % (list(self.ranges), ", negate=True" if self.negate else "")


class TemplateSet:
    """Keyword templates packed to the arrays of an ACMTemplateSpec.  `templates`: one sequence of cells per template
    (or bytes: literals only); a cell is an int (a literal symbol), ANY, or a SymbolClass.  `k`: a scalar or one
    budget per template; `terms`: one list of (keyword_id, offset, length) per template -- keyword keyword_id,
    `length` symbols long, is the piece at `offset`, on literal cells.  Symbols have `sym_size` bytes (default 1).
    from_templates() makes one by the canonical cut."""

    def __init__(self, templates, k, terms, sym_size=None):
        self.sym_size = int(sym_size) if sym_size is not None else 1
        dt = _SYM_DTYPE[self.sym_size]
        self.templates = [list(t) for t in templates]
        self.n_templates = self.n_targets = len(self.templates)
        ids, spell, cells = {}, [], []
        for t in self.templates:
            for c in t:
                if c is ANY:
                    spell.append(0)
                    cells.append(ACM_TEMPLATE_ANY)
                elif isinstance(c, SymbolClass):
                    spell.append(0)
                    cells.append(ids.setdefault(c, len(ids)))
                else:
                    spell.append(int(c))
                    cells.append(ACM_TEMPLATE_LITERAL)
        self.classes = list(ids)                                   # (a dict keeps the order of insertion: the ids)
        self.spell_data = np.array(spell, dtype=dt)
        self.cells = np.array(cells, dtype=np.uint32)
        self.spell_off = np.zeros(self.n_templates + 1, np.uint64)
        self.k = np.ascontiguousarray(np.broadcast_to(np.asarray(k, dtype=np.uint32), (self.n_templates,)))
        terms = [list(t) for t in terms]
        assert len(terms) == self.n_templates, "one list of terms per template"
        self.terms = np.array([tuple(int(x) for x in t) for p in terms for t in p], dtype=np.uint32).reshape(-1, 3)
        self.tgt_ptr = np.zeros(self.n_templates + 1, np.uint64)
        if self.templates:
            np.cumsum([len(t) for t in self.templates], out=self.spell_off[1:])
            np.cumsum([len(p) for p in terms], out=self.tgt_ptr[1:])
        self.ranges = np.array([x for c in self.classes for r in c.ranges for x in r], dtype=dt)
        self.cls_ptr = np.zeros(len(self.classes) + 1, np.uint64)
        if self.classes:
            np.cumsum([len(c.ranges) for c in self.classes], out=self.cls_ptr[1:])
        self.cls_flags = np.array([ACM_TEMPLATE_NEGATED if c.negate else 0 for c in self.classes], dtype=np.uint32)
        self.n_keywords = int(self.terms[:, 0].max()) + 1 if self.terms.size else 0
        ptr = lambda a: a.ctypes.data if a.size else None
        self.spec = TemplateSpec(ptr(self.spell_data), self.spell_off.ctypes.data, ptr(self.cells), ptr(self.k), ptr(self.terms), self.tgt_ptr.ctypes.data,
                                 self.n_templates, ptr(self.ranges), self.cls_ptr.ctypes.data, ptr(self.cls_flags), len(self.classes))

    @staticmethod
    def split(cells, k):
        """acm_templates_split(): the canonical cut of one template, [(offset, length)] of its k + 1 pieces; ValueError
        when the template has fewer than k + 1 literal cells"""
        words = np.array([ACM_TEMPLATE_ANY if c is ANY else 0 if isinstance(c, SymbolClass) else ACM_TEMPLATE_LITERAL for c in cells], dtype=np.uint32)
        pieces = []
        for j in range(int(k) + 1):
            o, n = C.c_uint64(0), C.c_uint64(0)
            if lib().acm_templates_split(words.ctypes.data if words.size else None, words.size, int(k), j, C.byref(o), C.byref(n)):
                raise ValueError("a template with %d literal cells cannot be cut into %d pieces"
                                 % (int((words == ACM_TEMPLATE_LITERAL).sum()), int(k) + 1))
            pieces.append((int(o.value), int(n.value)))
        return pieces

    @classmethod
    def from_templates(cls, machine, templates, k=0):
        """Every template is cut by the canonical cut (acm_templates_split: k + 1 pieces of one length on its literal
        runs); the distinct pieces `machine` does not hold yet are inserted as keywords in order of first appearance,
        those it holds keep their ids.  `k`: a scalar or one per template.  ValueError for a template with fewer than
        k + 1 literal cells.  Returns the TemplateSet (n_keywords = the machine's keywords afterwards)."""
        templates = [list(t) for t in templates]
        ks = [int(x) for x in np.broadcast_to(np.asarray(k), (len(templates),))]
        cuts = [cls.split(t, kk) for t, kk in zip(templates, ks)]   # (every template is cut before the machine grows)
        pieces = _PieceKeywords(machine)
        terms = [[(pieces.add(t[o:o + n]), o, n) for o, n in cut] for t, cut in zip(templates, cuts)]
        tset = cls(templates, ks, terms, sym_size=machine.sym_size)
        tset.n_keywords = machine.nb_keywords
        return tset

    def args(self):
        """(the ACMTemplateSpec by reference,) as the C calls take it"""
        return (C.byref(self.spec),)

    def check(self, n_keywords):
        """acm_templates_check(): raises ACMError (ACM_GPU_E_ARG) for a set the calls would refuse"""
        _check(lib().acm_templates_check(*self.args(), self.sym_size, int(n_keywords)), "acm_templates_check")


def templates_records(records, templateset, text, offsets=None, pos_base=0, n_keywords=None, out_capacity=None):
    """acm_templates_records(): the places where the templates of `templateset` (a TemplateSet) accept the text with
    at most k failing cells, among those the `records` seed, by the sequential pass on the host; arguments, order
    and return as approx_records(): (matches, dist) with the template's id as keyword_id."""
    return _set_records("acm_templates_records", records, templateset, text, offsets, pos_base, n_keywords, out_capacity)


_TEMPLATE_ESCAPES = {"n": 10, "t": 9, "r": 13, "f": 12, "v": 11, "0": 0}
_TEMPLATE_CLASSES = {"d": ((48, 57),), "w": ((48, 57), (65, 90), (95, 95), (97, 122)), "s": ((9, 13), (32, 32))}


def template(string):
    """The cells of a byte template written in a fixed-length subset of regular-expression syntax: literals, `.` (any
    byte), sets `[a-z0-9_]` and `[^...]`, `\\d` `\\w` `\\s` (ASCII; upper case negates, outside a set), `\\xHH`,
    `\\n \\t \\r \\f \\v \\0`, escaped punctuation, and `{n}` behind a cell.  Everything of variable length or
    without a width (`* + ? | ( ) {n,m} ^ $`) raises ValueError.  `string` is a str of code points below 256, or bytes."""
    s = string.decode("latin-1") if isinstance(string, (bytes, bytearray)) else str(string)
    if any(ord(c) > 255 for c in s):
        raise ValueError("a byte template holds code points below 256 only")

    def escape(i, in_set):
        """the cell (an int, or a tuple of ranges) of the escape whose letter is s[i], and the index behind it"""
        if i >= len(s):
            raise ValueError("a template ends inside an escape")
        c = s[i]
        if c == "x":
            if i + 3 > len(s) or any(h not in "0123456789abcdefABCDEF" for h in s[i + 1:i + 3]):
                raise ValueError("\\x takes two hex digits")
            return int(s[i + 1:i + 3], 16), i + 3
        if c in _TEMPLATE_CLASSES:
            return _TEMPLATE_CLASSES[c], i + 1
        if c.lower() in _TEMPLATE_CLASSES and not in_set:
            return SymbolClass(_TEMPLATE_CLASSES[c.lower()], negate=True), i + 1
        if c in _TEMPLATE_ESCAPES:
            return _TEMPLATE_ESCAPES[c], i + 1
        if c.isalnum() or c == "_":
            raise ValueError("the escape \\%s is not part of the template syntax" % c)
        return ord(c), i + 1

    cells, i = [], 0
    while i < len(s):
        c = s[i]
        if c in "*+?|()^$":
            raise ValueError("%r at %d: a template has one cell per symbol" % (c, i))
        if c == "{":
            j = s.find("}", i)
            if j < 0 or not s[i + 1:j].isdigit() or not cells:
                raise ValueError("a repeat at %d must be {n} behind a cell" % i)
            n = int(s[i + 1:j])
            if n == 0:
                cells.pop()
            else:
                cells.extend([cells[-1]] * (n - 1))
            i = j + 1
            continue
        if c == "}" or c == "]":
            raise ValueError("%r at %d stands alone" % (c, i))
        if c == ".":
            cells.append(ANY)
            i += 1
        elif c == "\\":
            cell, i = escape(i + 1, False)
            cells.append(SymbolClass(cell) if isinstance(cell, tuple) else cell)
        elif c == "[":
            i += 1
            negate = i < len(s) and s[i] == "^"
            i += negate
            ranges = []
            while i < len(s) and s[i] != "]":
                if s[i] == "[":
                    raise ValueError("a set inside a set at %d" % i)
                lo, i = escape(i + 1, True) if s[i] == "\\" else (ord(s[i]), i + 1)
                if isinstance(lo, tuple):
                    ranges.extend(lo)
                    continue
                hi = lo
                if i + 1 < len(s) and s[i] == "-" and s[i + 1] != "]":
                    hi, i = escape(i + 2, True) if s[i + 1] == "\\" else (ord(s[i + 1]), i + 2)
                    if isinstance(hi, tuple) or hi < lo:
                        raise ValueError("a range in a set ends below its begin, or on a class")
                ranges.append((lo, hi))
            if i >= len(s) or not ranges:
                raise ValueError("a set without an end, or an empty one")
            if len(ranges) > ACM_TEMPLATE_MAX_RANGES:
                raise ValueError("a set of more than %d ranges" % ACM_TEMPLATE_MAX_RANGES)
            cells.append(SymbolClass(ranges, negate))
            i += 1
        else:
            cells.append(ord(c))
            i += 1
    return cells


def hex_template(string):
    """The cells of a hex signature: tokens between blanks; `E2` is a literal byte, `??` ANY, `3?` the 16 bytes 0x30 to
    0x3F, `?3` the 16 bytes whose low nibble is 3, `[C0-CF]` a byte range.  ValueError for anything else."""
    hexd = "0123456789abcdefABCDEF"
    cells = []
    for tok in str(string).split():
        if len(tok) == 2 and tok[0] in hexd and tok[1] in hexd:
            cells.append(int(tok, 16))
        elif tok == "??":
            cells.append(ANY)
        elif len(tok) == 2 and tok[0] in hexd and tok[1] == "?":
            cells.append(SymbolClass([(int(tok[0], 16) << 4, (int(tok[0], 16) << 4) | 15)]))
        elif len(tok) == 2 and tok[0] == "?" and tok[1] in hexd:
            cells.append(SymbolClass([(hi << 4) | int(tok[1], 16) for hi in range(16)]))
        elif len(tok) == 7 and tok[0] == "[" and tok[3] == "-" and tok[6] == "]" and all(h in hexd for h in tok[1:3] + tok[4:6]) \
                and int(tok[1:3], 16) <= int(tok[4:6], 16):
            cells.append(SymbolClass([(int(tok[1:3], 16), int(tok[4:6], 16))]))
        else:
            raise ValueError("%r is no token of a hex signature" % tok)
    return cells


def _iupac():
    codes = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
             "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG"}
    cells = {c: ord(m) if len(m) == 1 else SymbolClass([ord(x) for x in m]) for c, m in codes.items()}
    cells["N"] = ANY
    return cells


IUPAC = _iupac()   # the 15 IUPAC nucleotide codes as cells over upper-case ASCII: [IUPAC[c] for c in "GGNRYCC"] is a template


def _delims(delims, sym_size, raw=False):
    """delimiters as a contiguous array of whole symbols: bytes are one symbol per byte, widened to the
    symbol size (b"\\n" is the symbol 10), unless `raw` (symbols without a numpy type: the bytes as they are)"""
    if raw or sym_size not in _SYM_DTYPE:
        d = np.frombuffer(bytes(delims), dtype=np.uint8) if isinstance(delims, (bytes, bytearray)) else np.ascontiguousarray(delims).reshape(-1).view(np.uint8)
        assert d.size % sym_size == 0
        return d, d.size // sym_size
    if isinstance(delims, (bytes, bytearray)):
        delims = np.frombuffer(bytes(delims), dtype=np.uint8)
    d = np.ascontiguousarray(np.asarray(delims).reshape(-1), dtype=_SYM_DTYPE[sym_size])
    return d, d.size


def split_offsets(text, delims=b"\n", runs=False, sym_size=None):
    """acm_split_offsets(): the offsets of the texts a buffer holds between its delimiter symbols, by
    the sequential pass on the host -- lines (a cut behind every delimiter) or, with runs, words (a cut
    behind every run of delimiters); an unterminated last text counts.  `text` is an array of symbols;
    with sym_size, raw bytes of symbols of that size, and `delims` raw bytes too.  Returns the
    n_texts + 1 offsets as a numpy uint64 array."""
    t = np.ascontiguousarray(text)
    sb = int(sym_size) if sym_size is not None else t.itemsize
    d, nd = _delims(delims, sb, raw=sym_size is not None)
    n_sym = t.size * t.itemsize // sb
    flags = ACM_SPLIT_RUNS if runs else ACM_SPLIT_EVERY
    n = C.c_uint64(0)
    _check(lib().acm_split_offsets(t.ctypes.data if t.size else None, n_sym, sb, d.ctypes.data, nd, flags, None, 0, C.byref(n)), "acm_split_offsets")
    off = np.zeros(int(n.value) + 1, np.uint64)
    _check(lib().acm_split_offsets(t.ctypes.data if t.size else None, n_sym, sb, d.ctypes.data, nd, flags, off.ctypes.data, int(n.value), C.byref(n)),
           "acm_split_offsets")
    return off


def _word_ranges(ranges, sym_size):
    """a word set -- inclusive (lo, hi) pairs of symbol values -- as the contiguous 2 * n_ranges symbols the C calls take"""
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.uint64).reshape(-1, 2), dtype=_SYM_DTYPE[sym_size]).reshape(-1)
    return r, r.size // 2


_WORD_FLAGS = {"left": ACM_WORDS_LEFT, "right": ACM_WORDS_RIGHT, "both": ACM_WORDS_BOTH}


def _word_flags(flags):
    return _WORD_FLAGS[flags] if isinstance(flags, str) else int(flags)


def words_records(text, records, offsets=None, ranges=ASCII_WORD, flags="both", pos_base=0, sym_size=None):
    """acm_words_records(): the whole-word records of `records` (RECORD_DTYPE, any order) over `text`
    (an array of symbols; with sym_size, raw bytes of symbols of that size), by the sequential pass on
    the host: a record is kept when the symbol in front of it ("left"), behind it ("right") or both
    ("both": grep -w) is no word symbol or lies outside the record's text.  `ranges` is the word set,
    inclusive (lo, hi) pairs; `offsets` (n_texts + 1 entries) cuts the buffer into texts.  Returns a
    new array in the order of the input; `records` is not changed."""
    t = np.ascontiguousarray(text)
    sb = int(sym_size) if sym_size is not None else t.itemsize
    r, nr = _word_ranges(ranges, sb)
    a = np.array(records, dtype=RECORD_DTYPE, copy=True).reshape(-1)
    off = np.ascontiguousarray(offsets, dtype=np.uint64) if offsets is not None else None
    n = C.c_uint64(0)
    _check(lib().acm_words_records(_ptr(t), t.size * t.itemsize // sb, sb, int(pos_base), *_cut(off), r.ctypes.data, nr, _word_flags(flags), _ptr(a),
                                   a.size, C.byref(n)), "acm_words_records")
    return a[:n.value]


_CHARS_UNITS = {"codepoints": ACM_CHARS_CODEPOINTS, "utf16": ACM_CHARS_UTF16, "utf-16": ACM_CHARS_UTF16}


def _chars_unit(unit):
    return _CHARS_UNITS[unit] if isinstance(unit, str) else int(unit)


def chars_positions(text, positions, offsets=None, unit="codepoints"):
    """acm_chars_positions(): the byte positions `positions` (0 .. len(text)) of the UTF-8 bytes `text` (bytes or a
    uint8 array) in code points ("codepoints") or UTF-16 code units ("utf16"), counted from the beginning of the
    text that holds each -- `offsets` (n_texts + 1 entries) cuts the buffer into texts --, by the sequential
    definition on the host.  Returns a np.uint64 array."""
    t = np.frombuffer(bytes(text), np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)
    p = np.ascontiguousarray(positions, dtype=np.uint64).reshape(-1)
    off = np.ascontiguousarray(offsets, dtype=np.uint64) if offsets is not None else None
    out = np.zeros(p.size, np.uint64)
    _check(lib().acm_chars_positions(_ptr(t), t.size, *_cut(off), _chars_unit(unit), _ptr(p), p.size, _ptr(out)), "acm_chars_positions")
    return out


def chars_records(text, records, offsets=None, unit="codepoints", pos_base=0):
    """acm_chars_records(): where every record of `records` (RECORD_DTYPE, any order) over the UTF-8 bytes `text`
    lies in code points or UTF-16 code units (see chars_positions), by the sequential definition on the host.
    Returns (char_start, char_len, edge): np.uint64, np.uint32 and np.uint8 arrays, one entry per record;
    edge 0 says that the record begins and ends between characters (include/acm_chars.h)."""
    t = np.frombuffer(bytes(text), np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)
    a = np.ascontiguousarray(records, dtype=RECORD_DTYPE).reshape(-1)
    off = np.ascontiguousarray(offsets, dtype=np.uint64) if offsets is not None else None
    start, length, edge = np.zeros(a.size, np.uint64), np.zeros(a.size, np.uint32), np.zeros(a.size, np.uint8)
    _check(lib().acm_chars_records(_ptr(t), t.size, int(pos_base), *_cut(off), _chars_unit(unit), _ptr(a), a.size, start.ctypes.data,
                                   length.ctypes.data, edge.ctypes.data), "acm_chars_records")
    return start, length, edge


def _chars_host_call(fn, what, before, cap, fixed):
    """fn(*before, records, char_start, char_len, edge, cap, n) in the room loop: (records, char_start, char_len, edge)"""
    def call(cap):
        out = (np.zeros(cap, dtype=RECORD_DTYPE), np.zeros(cap, np.uint64), np.zeros(cap, np.uint32), np.zeros(cap, np.uint8))
        n = C.c_uint64(0)
        return fn(*before, *[a.ctypes.data for a in out], cap, C.byref(n)), n.value, out
    out, n, _ = _room_call(call, what, cap, fixed)
    return tuple(a[:n] for a in out)


class Snippets:
    """What the context calls return: the text around the matches, packed.  out (the snippets side by
    side, in the text's own symbols), out_offsets (n_snippets + 1 offsets into `out`), snip_lo (the
    buffer index of every snippet's first symbol), snip_text (the text that holds it), rec_snip (the
    snippet every record lies in, ACM_CONTEXT_NONE for a record that spans a cut) and rec_at (where
    the match begins in `out`, -1 for such a record): numpy arrays cut to size from the host calls;
    device tensors with room for every record from the Plan calls -- their first n_snippets (+ 1) or
    `count` entries and out_symbols symbols count.  `records` are the records the windows were made
    round.  n_snippets, out_symbols and count are Python ints (the Plan calls synchronise to read
    them): count > capacity says that the scan overflowed (n_snippets = out_symbols = 0 then),
    out_symbols > out_capacity is the room the output needs.  snippets[j] is snippet j, len() their number."""

    def __init__(self, out, out_offsets, snip_lo, snip_text, rec_snip, rec_at, n_snippets, out_symbols, out_capacity=None, records=None, count=None,
                 sym_size=None):
        self.out, self.out_offsets, self.snip_lo, self.snip_text, self.rec_snip, self.rec_at = out, out_offsets, snip_lo, snip_text, rec_snip, rec_at
        self.n_snippets, self.out_symbols, self.out_capacity, self.records, self.count = n_snippets, out_symbols, out_capacity, records, count
        self.sym_size = sym_size            # bytes per symbol; None: one element of `out` per symbol
        self.offsets = None                 # Plan.grep_context_lines: the n_texts + 1 offsets the buffer was cut at

    def __len__(self):
        return self.n_snippets

    def __getitem__(self, j):
        if self.out is None or not -self.n_snippets <= j < self.n_snippets:
            raise IndexError(j)
        j %= self.n_snippets
        per = 1 if self.sym_size is None else self.sym_size // (self.out.element_size() if hasattr(self.out, "element_size") else self.out.itemsize)
        return self.out[int(self.out_offsets[j]) * per:int(self.out_offsets[j + 1]) * per]


_CONTEXT_UNITS = {"symbols": ACM_CONTEXT_SYMBOLS, "texts": ACM_CONTEXT_TEXTS}


def _context_flags(unit, merge):
    return (_CONTEXT_UNITS[unit] if isinstance(unit, str) else int(unit)) | (ACM_CONTEXT_MERGE if merge else ACM_CONTEXT_EACH)


def _context_host_call(call, what, t, sym_size, room, grow, gather, out_capacity):
    """the host context calls: numpy in, a Snippets of numpy arrays out.  `call` takes the record room and (out,
    out_capacity, out_symbols, n_snippets, snip_lo, out_offsets, snip_text, rec_snip, rec_at) and returns (rc, the
    records, their number).  Each of the two overflows is repeated once with the size the call reports: the records'
    when `grow`, the output's when out_capacity is None."""
    cap = int(out_capacity) if out_capacity is not None else 0
    for attempt in (0, 1, 2):
        snip_lo, out_off = np.zeros(max(room, 1), np.uint64), np.zeros(room + 1, np.uint64)
        snip_text, rec_snip, rec_at = np.zeros(max(room, 1), np.uint32), np.zeros(max(room, 1), np.uint32), np.zeros(max(room, 1), np.int64)
        out = np.zeros(max(cap * sym_size // t.itemsize, 1), dtype=t.dtype) if gather else None
        sym, ns = C.c_uint64(0), C.c_uint64(0)
        rc, records, m = call(room, out.ctypes.data if gather else None, cap if gather else 0, C.byref(sym), C.byref(ns), snip_lo.ctypes.data,
                              out_off.ctypes.data, snip_text.ctypes.data, rec_snip.ctypes.data, rec_at.ctypes.data)
        if rc == ACM_GPU_E_OVERFLOW and m > room and grow and attempt < 2:
            room, grow = m, False
            continue
        if rc == ACM_GPU_E_OVERFLOW and m <= room and out_capacity is None and int(sym.value) > cap and attempt < 2:
            cap = int(sym.value)
            continue
        _check(rc, what)
        k, n = int(ns.value), int(sym.value)
        return Snippets(out[:n * sym_size // t.itemsize] if gather else None, out_off[:k + 1], snip_lo[:k], snip_text[:k], rec_snip[:m], rec_at[:m],
                        k, n, cap, records, m, sym_size)


def context_records(text, records, offsets=None, before=0, after=0, unit="symbols", merge=True, pos_base=0, sym_size=None, gather=True,
                    out_capacity=None):
    """acm_context_records(): the text round the matches `records` (RECORD_DTYPE) of `text` (an array of
    symbols; with sym_size, raw bytes of symbols of that size), by the sequential pass on the host: every
    match with `before` symbols in front of it and `after` behind it, clipped to its text -- with unit
    "texts", its whole text with that many texts in front and behind (grep -B / -A).  merge: windows that
    overlap or touch become one snippet (grep -C; the records' end_pos must not decrease); else one
    snippet per record, in the order of the input.  `offsets` (n_texts + 1 entries) cuts the buffer into
    texts.  Returns a Snippets of numpy arrays."""
    t = np.ascontiguousarray(text)
    sb = int(sym_size) if sym_size is not None else t.itemsize
    a = np.ascontiguousarray(np.asarray(records, dtype=RECORD_DTYPE).reshape(-1))
    off = np.ascontiguousarray(offsets, dtype=np.uint64) if offsets is not None else None
    flags = _context_flags(unit, merge)

    def call(room, *outputs):
        return lib().acm_context_records(_ptr(t), t.size * t.itemsize // sb, sb, int(pos_base), *_cut(off), _ptr(a), a.size, int(before), int(after),
                                         flags, *outputs), a, a.size
    return _context_host_call(call, "acm_context_records", t, sb, a.size, False, gather, out_capacity)


def _context_scan_call(fn, head, t, n_sym, off, before, after, flags):
    """acm_context / acm_gpu_scan_context_host as _context_host_call's `call`: a record room of the call's own"""
    def call(room, *outputs):
        rec = np.zeros(max(room, 1), dtype=RECORD_DTYPE)
        n = C.c_uint64(0)
        rc = fn(*head, t.ctypes.data if t.size else None, n_sym, *off, rec.ctypes.data, room, C.byref(n), int(before), int(after), flags, *outputs)
        return rc, rec[:min(int(n.value), room)], int(n.value)
    return call


_ANCHORED_MODES = {"prefixes": ACM_ANCHORED_PREFIXES, "longest": ACM_ANCHORED_LONGEST, "whole": ACM_ANCHORED_WHOLE}


def _anchored_mode(mode):
    return _ANCHORED_MODES[mode] if isinstance(mode, str) else int(mode)


def anchored_records(records, offsets, mode="prefixes"):
    """acm_anchored_records(): ANCHORED of a batch's records (RECORD_DTYPE, canonical order) under
    `offsets` by the sequential pass on the host -- mode "prefixes" (the keywords every text begins
    with), "longest" (the longest of them) or "whole" (the keyword that spells the whole text).
    Returns new arrays (records, text_id, first); `records` is not changed."""
    a = np.array(records, dtype=RECORD_DTYPE, copy=True).reshape(-1)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    assert off.size >= 1, "offsets has n_texts + 1 entries"
    tid = np.zeros(max(a.size, 1), dtype=np.uint32)
    first = np.zeros(off.size, dtype=np.uint64)
    n = C.c_uint64(0)
    _check(lib().acm_anchored_records(off.ctypes.data, off.size - 1, _anchored_mode(mode), a.ctypes.data if a.size else None, a.size,
                                      tid.ctypes.data, first.ctypes.data, C.byref(n)), "acm_anchored_records")
    return a[:n.value], tid[:n.value], first


def _anchored_host_call(fn, what, handle, t, off, mode, capacity):
    """the host-memory anchored calls (plan or machine): (records, text_id, first); an overflow is
    repeated once with the size the call reports unless `capacity` was given"""
    n_texts = off.size - 1
    return _batch_records_host_call(fn, what, (handle, _ptr(t), off.ctypes.data, n_texts, _anchored_mode(mode)), n_texts,
                                    int(capacity) if capacity is not None else max(n_texts, 1), capacity is not None)


def _batch_records_host_call(fn, what, before, n_texts, cap, fixed=False):
    """fn(*before, out, text_id, first, cap, n) in the room loop, for the host calls that give the records of a
    batch: (records, text_id, first)"""
    def call(cap):
        out = np.zeros(max(cap, 1), dtype=RECORD_DTYPE)
        tid = np.zeros(max(cap, 1), dtype=np.uint32)
        first = np.zeros(n_texts + 1, dtype=np.uint64)
        n = C.c_uint64(0)
        return fn(*before, out.ctypes.data, tid.ctypes.data, first.ctypes.data, cap, C.byref(n)), n.value, (out, tid, first)
    (out, tid, first), n, _ = _room_call(call, what, cap, fixed)
    return out[:n], tid[:n], first


def _segment_host_call(fn, what, before, cost, gap_cost, cap, fixed):
    """acm_segment / acm_gpu_scan_segment_host: fn(*before, the cost table, gap_cost, out, cap, n, sums) in the room
    loop; (records, sums)"""
    c, cp = _costs(cost)

    def call(cap):
        out = np.zeros(cap, dtype=RECORD_DTYPE)
        n = C.c_uint64(0)
        sums = np.zeros(2, np.uint64)
        return fn(*before, cp, c.size, int(gap_cost), out.ctypes.data, cap, C.byref(n), sums.ctypes.data), n.value, (out, sums)
    (out, sums), n, _ = _room_call(call, what, cap, fixed)
    return out[:n], (int(sums[0]), int(sums[1]))


def _replace_host_call(fn, what, handle, t, sym_size, replacements, fill, out_capacity):
    """acm_replace / acm_gpu_scan_replace_host: numpy in, (the new text, the number of matches replaced) out.  An
    output overflow is repeated once with the size the call reports when out_capacity is None."""
    n_sym = t.size * t.itemsize // sym_size
    data, off, nk = replacement_table(replacements, sym_size, fill)

    def call(cap):
        out = np.zeros(max(cap * sym_size // t.itemsize, 1), dtype=t.dtype)
        need, m = C.c_uint64(0), C.c_uint64(0)
        rc = fn(handle, _ptr(t), n_sym, data.ctypes.data, _opt(off), nk, out.ctypes.data, cap, C.byref(need), C.byref(m))
        return rc, need.value, (out, m)
    (out, m), need, _ = _room_call(call, what, int(out_capacity) if out_capacity is not None else n_sym + 1024, out_capacity is not None)
    return out[:need * sym_size // t.itemsize], int(m.value)


def _tokenize_host_call(fn, what, handle, t, sym_size, off, mode, gap_base, tok_of, token_capacity):
    """acm_tokenize / acm_gpu_scan_tokens_host: numpy in, a Tokens of numpy arrays out; `off` None: one text"""
    n_sym = t.size * t.itemsize // sym_size
    table, nk = _tok_of(tok_of)
    md = _token_mode(mode)
    off_ptr, n_texts = _cut(off)

    def call(ids, start, length, cap, need, first, m):
        return fn(handle, _ptr(t), n_sym, off_ptr, n_texts, _opt(table), nk, int(gap_base), md, _opt(ids), _opt(start), _opt(length), cap,
                  C.byref(need), _opt(first), C.byref(m))
    return _tokens_host_call(call, what, n_texts, off is not None, token_capacity)


def _lookup_host_call(fn, what, handle, t, off):
    """the host-memory lookup calls (plan or machine): (whole_id, prefix_id, prefix_len), one entry per text"""
    n_texts = off.size - 1
    res = [np.zeros(max(n_texts, 1), dtype=np.uint32) for _ in range(3)]
    _check(fn(handle, t.ctypes.data if t.size else None, off.ctypes.data, n_texts, *[r.ctypes.data for r in res]), what)
    return tuple(r[:n_texts] for r in res)


def _grep_lines_host_call(fn, what, handle, t, sym_size, d, nd, runs, invert, gather):
    """acm_gpu_grep_lines_host / acm_grep_lines: numpy in, a Grepped of numpy arrays out.  A first call
    with no room for a text learns n_texts (it ends behind the split's count), the second has room."""
    n_sym = t.size * t.itemsize // sym_size
    sflags, gflags = ACM_SPLIT_RUNS if runs else ACM_SPLIT_EVERY, ACM_GREP_INVERT if invert else ACM_GREP_MATCHING
    nt, nk, total, sym = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    tp = t.ctypes.data if t.size else None
    one = np.zeros(1, np.uint64)
    rc = fn(handle, tp, n_sym, d.ctypes.data, nd, sflags, gflags, C.byref(nt), C.byref(nk), C.byref(total), None, 0, C.byref(sym), 0,
            one.ctypes.data, None, None, None)
    if rc != ACM_GPU_E_OVERFLOW:
        _check(rc, what)
    n = int(nt.value)
    off, out_off = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    hits, kept = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint32)
    out = np.zeros(max(n_sym * sym_size // t.itemsize, 1), dtype=t.dtype) if gather else None       # the kept texts never need more than all
    _check(fn(handle, tp, n_sym, d.ctypes.data, nd, sflags, gflags, C.byref(nt), C.byref(nk), C.byref(total), out.ctypes.data if gather else None,
              n_sym if gather else 0, C.byref(sym), n, off.ctypes.data, hits.ctypes.data, kept.ctypes.data, out_off.ctypes.data), what)
    assert int(nt.value) == n
    k, s = int(nk.value), int(sym.value)
    return Grepped(hits[:n], kept[:k], k, int(total.value), None, out[:s * sym_size // t.itemsize] if gather else None, out_off[:k + 1], s, n_sym,
                   offsets=off, n_texts=n)


class FlatTables(_Owner):
    """Host snapshot of the machine's flattened goto/failure/output tables (acm_flatten)."""

    def __init__(self, handle):
        self._h = handle
        L = lib()
        info = FlatInfo()
        L.acm_flat_info(handle, C.byref(info))
        self.info = info
        v = FlatView()
        L.acm_flat_view(handle, C.byref(v))
        n, ne = info.n_states, info.n_edges

        def arr(p, cnt):
            return np.ctypeslib.as_array(p, shape=(cnt,)).copy() if cnt else np.zeros(0, np.uint32)
        self.row_ptr = arr(v.row_ptr, n + 1)
        self.edge_sym = arr(v.edge_sym, ne)
        self.edge_next = arr(v.edge_next, ne)
        self.fail = arr(v.fail, n)
        self.depth = arr(v.depth, n)
        self.nb_outputs = arr(v.nb_outputs, n)
        self.term_kw = arr(v.term_kw, n)
        self.out_link = arr(v.out_link, n)
        self.depth_start = arr(v.depth_start, info.lmax + 2)
        self.kw_state = arr(v.kw_state, info.n_keywords)
        # comparator-class machines (acm_flatten_classes): class table and the dictionary's own letters
        self.n_classes = int(v.n_classes)
        self.class_map = np.ctypeslib.as_array(v.class_map, shape=(v.class_entries,)).copy() if v.class_entries else None
        self.edge_letter = arr(v.edge_letter, ne) if v.class_entries else None
        # 8-byte symbols: edge_sym = 1 + index into keys64 (the dictionary's distinct symbols, ascending)
        self.keys64 = np.ctypeslib.as_array(v.keys64, shape=(v.n_keys64,)).copy() if v.n_keys64 else None
        # comparator classes of 4-byte symbols: the dictionary's distinct symbols, their classes (1 .. n_classes),
        # one symbol per class in comparator order
        self.keys32 = arr(v.keys32, v.n_keys32) if v.n_keys32 else None
        self.keys32_class = arr(v.keys32_class, v.n_keys32) if v.n_keys32 else None
        self.class_rep32 = arr(v.class_rep32, v.n_classes) if v.n_keys32 else None
        if v.n_keys32:
            self.edge_letter = arr(v.edge_letter, ne)

    def dense_rows(self, n_rows=None, entry_bytes=None):
        info = self.info
        n_rows = info.n_states if n_rows is None else n_rows
        entry_bytes = (2 if info.n_states <= 32768 else 4) if entry_bytes is None else entry_bytes
        out = np.zeros(n_rows * info.width, dtype=np.uint16 if entry_bytes == 2 else np.uint32)
        _check(lib().acm_flat_dense_rows(self._h, n_rows, entry_bytes, out.ctypes.data), "acm_flat_dense_rows")
        return out.reshape(n_rows, info.width)

    # ---- serialised form (acm_flat_to_blob / acm_flat_from_blob / acm_flat_save / acm_flat_load)
    def to_bytes(self):
        L = lib()
        n = L.acm_flat_blob_bytes(self._h)
        buf = (C.c_ubyte * n)()
        _check(L.acm_flat_to_blob(self._h, buf, n), "acm_flat_to_blob")
        return bytes(buf)

    @classmethod
    def from_bytes(cls, blob):
        h = C.c_void_p()
        buf = (C.c_ubyte * max(len(blob), 1)).from_buffer_copy(blob if len(blob) else b"\0")
        _check(lib().acm_flat_from_blob(buf, len(blob), C.byref(h)), "acm_flat_from_blob")
        return cls(h)

    def save(self, path):
        _check(lib().acm_flat_save(self._h, os.fsencode(path)), "acm_flat_save")

    @classmethod
    def load(cls, path):
        h = C.c_void_p()
        _check(lib().acm_flat_load(os.fsencode(path), C.byref(h)), "acm_flat_load")
        return cls(h)

    def keyword(self, keyword_id):
        """Spelling of a keyword from the tables alone: numpy array of symbols."""
        sb = self.info.sym_bytes
        n = C.c_uint32(0)
        L = lib()
        _check(L.acm_flat_keyword(self._h, keyword_id, None, 0, C.byref(n)), "acm_flat_keyword")
        out = np.zeros(n.value, dtype={1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[sb])
        _check(L.acm_flat_keyword(self._h, keyword_id, out.ctypes.data, n.value, C.byref(n)), "acm_flat_keyword")
        return out

    def plan(self, device=0):
        """Device plan straight from the tables (no machine needed: acm_gpu_plan_create_flat)."""
        h = C.c_void_p()
        _check(lib().acm_gpu_plan_create_flat(self._h, device, C.byref(h)), "acm_gpu_plan_create_flat")
        return Plan(h, self.info.sym_bytes)

    def close(self):
        if self._h:
            lib().acm_flat_release(self._h)
            self._h = None


class Machine(_Owner):
    """An ACMachine over fixed-size symbols compared with ACM_CMP_DEFAULT (reference
    aho_corasick.h:35,45), i.e. what `acm_create (ACM_CMP_DEFAULT, &(size_t){ sym_size }, 0)` returns.
    With `cmp` (a C function pointer of type CMP_TYPE, e.g. ctypes.cast(lib.sym, c_void_p)) the
    machine orders its alphabet with that comparator instead; such a machine reaches the GPU through
    flatten_classes() / plan_classes() when its symbols are 1 or 2 bytes wide."""

    def __init__(self, sym_size=1, cmp=None, cmp_arg=None):
        L = lib()
        self.L = L
        self.sym_size = sym_size
        self.custom_cmp = cmp is not None
        if cmp is None:
            self._arg = C.c_size_t(sym_size)
            cmp = C.c_void_p.in_dll(L, "ACM_CMP_DEFAULT")
            cmp_arg = C.cast(C.pointer(self._arg), C.c_void_p)
        self.handle = L.acm_create(cmp, cmp_arg, None)
        self._keep = []  # letters must outlive the machine (reference aho_corasick.h:39-43)
        self.lmax = 0

    def close(self):
        if self.handle:
            self.L.acm_release(self.handle)
            self.handle = None

    def _symbols(self, x):
        if isinstance(x, (bytes, bytearray)):
            x = np.frombuffer(bytes(x), dtype=np.uint8)
        return np.ascontiguousarray(x, dtype=_SYM_DTYPE[self.sym_size])

    def _text(self, text):
        """(the text as a contiguous array, its number of symbols) as the one-text calls take it"""
        t = np.ascontiguousarray(text) if self.sym_size not in _SYM_DTYPE else self._symbols(text)
        return t, t.size * t.itemsize // self.sym_size

    def _pack_texts(self, texts):
        """a list of texts (bytes or arrays of symbols) side by side in one array, and their n + 1 offsets"""
        def symbols(t):
            if self.sym_size in _SYM_DTYPE:
                return self._symbols(t)
            return np.frombuffer(bytes(t), dtype=np.uint8) if isinstance(t, (bytes, bytearray)) else np.ascontiguousarray(t)
        parts = [symbols(t).reshape(-1) for t in texts]
        offsets = np.zeros(len(parts) + 1, dtype=np.uint64)
        if parts:
            np.cumsum([p.size * p.itemsize // self.sym_size for p in parts], out=offsets[1:])
        dtype = _SYM_DTYPE.get(self.sym_size, np.uint8)
        packed = np.concatenate([p.view(dtype) for p in parts]) if parts else np.zeros(0, dtype)
        return packed, offsets

    def add_keyword(self, symbols, value=None):
        """acm_insert_letter_of_keyword per symbol then acm_insert_end_of_keyword.  Returns the
        previous value pointer (None when the keyword had no value yet)."""
        arr = self._symbols(symbols)
        assert arr.size > 0
        self._keep.append(arr)
        L = self.L
        cur = C.c_void_p(L.acm_initiate(self.handle))
        base = arr.ctypes.data
        for i in range(arr.size):
            L.acm_insert_letter_of_keyword(C.byref(cur), base + i * self.sym_size)
        self.lmax = max(self.lmax, int(arr.size))
        return L.acm_insert_end_of_keyword(C.byref(cur), value, None)

    def add_keywords_packed(self, data, offsets, ids_as_values=False):
        """ids_as_values: register value = (void *)(keyword_id + 1) with every keyword, so that a
        caller of the per-symbol API can tell the keywords apart (the reference has no keyword id;
        its MatchHolder.value is the only per-keyword datum, aho_corasick.h:23-28)."""
        data = self._symbols(data)
        self._keep.append(data)
        L = self.L
        base, ss = data.ctypes.data, self.sym_size
        ins, end, init = L.acm_insert_letter_of_keyword, L.acm_insert_end_of_keyword, L.acm_initiate
        nbk = L.acm_nb_keywords
        for k in range(len(offsets) - 1):
            cur = C.c_void_p(init(self.handle))
            ref = C.byref(cur)
            for i in range(int(offsets[k]), int(offsets[k + 1])):
                ins(ref, base + i * ss)
            end(ref, (nbk(self.handle) + 1) if ids_as_values else None, None)
            self.lmax = max(self.lmax, int(offsets[k + 1] - offsets[k]))

    @property
    def nb_keywords(self):
        return int(self.L.acm_nb_keywords(self.handle))

    def match_loop(self, text):
        """The reference's caller loop through the per-symbol host API (examples/test.c:17-23):
        returns records (end_pos, length) and, per record, the matched spelling.  Slow (ctypes
        call per symbol): API-parity tests only."""
        t = self._symbols(text)
        L = self.L
        cur = C.c_void_p(L.acm_initiate(self.handle))
        h = MatchHolder()
        L.acm_matcher_init(C.byref(h))
        out = []
        base = t.ctypes.data
        ptr_t = C.POINTER({1: C.c_uint8, 2: C.c_uint16, 4: C.c_uint32, 8: C.c_uint64}[self.sym_size])
        for i in range(t.size):
            nb = L.acm_match(C.byref(cur), base + i * self.sym_size)
            for j in range(nb):
                L.acm_get_match(cur, j, C.byref(h))
                word = tuple(C.cast(h.letters[k], ptr_t)[0] for k in range(h.length))
                out.append((i, int(h.length), word, h.value))
        L.acm_matcher_release(C.byref(h))
        return out

    def keyword(self, keyword_id):
        """(symbols tuple, value pointer) of a keyword id, through acm_get_keyword."""
        h = MatchHolder()
        self.L.acm_matcher_init(C.byref(h))
        _check(self.L.acm_get_keyword(self.handle, keyword_id, C.byref(h)), "acm_get_keyword")
        ptr_t = C.POINTER({1: C.c_uint8, 2: C.c_uint16, 4: C.c_uint32, 8: C.c_uint64}[self.sym_size])
        word = tuple(C.cast(h.letters[k], ptr_t)[0] for k in range(h.length))
        value = h.value
        self.L.acm_matcher_release(C.byref(h))
        return word, value

    def flatten(self):
        h = C.c_void_p()
        _check(self.L.acm_flatten(self.handle, C.byref(h)), "acm_flatten")
        return FlatTables(h)

    def plan(self, device=0):
        h = C.c_void_p()
        _check(self.L.acm_gpu_plan_create(self.handle, device, C.byref(h)), "acm_gpu_plan_create")
        return Plan(h, self.sym_size)

    # ---- machines with a custom comparator (acm_flatten_classes / acm_gpu_plan_create_classes)
    def flatten_classes(self):
        h = C.c_void_p()
        _check(self.L.acm_flatten_classes(self.handle, self.sym_size, C.byref(h)), "acm_flatten_classes")
        return FlatTables(h)

    def plan_classes(self, device=0):
        h = C.c_void_p()
        _check(self.L.acm_gpu_plan_create_classes(self.handle, self.sym_size, device, C.byref(h)), "acm_gpu_plan_create_classes")
        return Plan(h, self.sym_size)

    def set_symbol_bytes(self, sym_bytes):
        """acm_set_symbol_bytes(): the symbol size of a machine with a comparator of its own."""
        _check(self.L.acm_set_symbol_bytes(self.handle, sym_bytes), "acm_set_symbol_bytes")

    @property
    def scan_path(self):
        """acm_scan_path(): 1 GPU, 2 GPU over comparator classes, 3 the caller loop on the host, 0 none yet."""
        return int(self.L.acm_scan_path(self.handle))

    def scan_host(self, text, capacity=None):
        """acm_scan(): host buffers in, canonical records out (GPU inside; the host loop for machines
        the GPU cannot take by their nature: scan_path says which)."""
        t, n_sym = self._text(text)
        return _records_host_call(self.L.acm_scan, "acm_scan", (self.handle, t.ctypes.data, n_sym),
                                  int(capacity) if capacity is not None else max(1024, t.size // 64), capacity is not None, repeats=None)

    def root(self):
        """The cursor of a scan that has seen nothing yet (acm_initiate): what scan_from() and the
        per-symbol acm_match start from."""
        return C.c_void_p(self.L.acm_initiate(self.handle))

    def scan_from(self, cursor, text, capacity=None):
        """acm_scan_from(): scan_host() continued from `cursor` (root(), or what an earlier scan_from
        or acm_match left).  Returns (records, cursor afterwards): end_pos is the index in `text`, a
        keyword cut by the boundary between two texts is found.  `cursor` itself is not changed."""
        t, n_sym = self._text(text)

        def call(cap):
            out = np.zeros(cap, dtype=RECORD_DTYPE)
            n = C.c_uint64(0)
            cur = C.c_void_p(cursor.value)
            return self.L.acm_scan_from(self.handle, C.byref(cur), t.ctypes.data, n_sym, out.ctypes.data, cap, C.byref(n)), n.value, (out, cur)
        (out, cur), n, _ = _room_call(call, "acm_scan_from", int(capacity) if capacity is not None else max(1024, t.size // 64),
                                      capacity is not None, repeats=None)
        return out[:n], cur

    def scan_batch(self, texts, capacity=None):
        """acm_scan_batch(): a list of texts (bytes or arrays of symbols), each scanned from the root
        on its own in ONE call.  Returns a list with one record array per text, end_pos relative to
        the text's own first symbol -- what scan_host() gives for each of them alone."""
        packed, offsets = self._pack_texts(texts)
        n_texts = offsets.size - 1

        def call(cap):
            out = np.zeros(cap, dtype=RECORD_DTYPE)
            first = np.zeros(n_texts + 1, dtype=np.uint64)
            n = C.c_uint64(0)
            rc = self.L.acm_scan_batch(self.handle, packed.ctypes.data, offsets.ctypes.data, n_texts, out.ctypes.data, None, first.ctypes.data, cap,
                                       C.byref(n))
            return rc, n.value, (out, first)
        (out, first), _, _ = _room_call(call, "acm_scan_batch", int(capacity) if capacity is not None else max(1024, int(offsets[-1]) // 64),
                                        capacity is not None, repeats=None)
        res = []
        for t in range(n_texts):
            r = out[int(first[t]):int(first[t + 1])].copy()
            r["end_pos"] -= offsets[t]
            res.append(r)
        return res

    def scan_anchored(self, texts, mode="prefixes", capacity=None):
        """acm_scan_anchored(): the keywords every text of a list begins with (mode "prefixes"), the
        longest of them ("longest") or the keyword that spells the whole text ("whole": `grep -x`).
        Returns (records, text_id, first) as scan_batch's packed form: end_pos = the index in the
        packed buffer, records [first[t], first[t + 1]) are those of text t."""
        packed, offsets = self._pack_texts(texts)
        return _anchored_host_call(self.L.acm_scan_anchored, "acm_scan_anchored", self.handle, packed, offsets, mode, capacity)

    def lookup(self, texts):
        """acm_lookup(): one answer per text of a list -- (whole_id, prefix_id, prefix_len): the id of
        the keyword that spells the whole text, the id and the length of the longest keyword the text
        begins with; ACM_LOOKUP_NONE / 0 where there is none.  whole_id is a column's dictionary code."""
        packed, offsets = self._pack_texts(texts)
        return _lookup_host_call(self.L.acm_lookup, "acm_lookup", self.handle, packed, offsets)

    def tally(self, text, tally=None):
        """acm_tally(): how often every keyword occurs in `text`.  Returns (np.uint64 array with one
        counter per keyword, number of matches).  `tally` (an earlier call's array, at least
        nb_keywords entries) is ADDED TO in place; keyword(k) gives the spelling of counter k."""
        t, n_sym = self._text(text)
        if tally is None:
            tally = np.zeros(self.nb_keywords, dtype=np.uint64)
        assert tally.dtype == np.uint64 and tally.flags.c_contiguous
        total = C.c_uint64(0)
        _check(self.L.acm_tally(self.handle, t.ctypes.data, n_sym, tally.ctypes.data, tally.size, C.byref(total)), "acm_tally")
        return tally, int(total.value)

    def select(self, text, capacity=None):
        """acm_select(): the leftmost-longest non-overlapping matches of `text` in canonical order --
        the one tiling a replacer, a redactor or a tokeniser acts on.  `capacity` must hold ALL
        matches (they are found first); by default an overflow is repeated once with the size the
        call reports."""
        t, n_sym = self._text(text)
        return _records_host_call(self.L.acm_select, "acm_select", (self.handle, t.ctypes.data, n_sym),
                                  int(capacity) if capacity is not None else max(1024, t.size // 64), capacity is not None)

    def segment(self, text, cost, gap_cost, capacity=None):
        """acm_segment(): the minimum-cost tiling of `text` by the keywords in canonical order, under
        cost[keyword_id] per match taken and gap_cost per uncovered symbol (include/acm_segment.h).
        `capacity` must hold ALL matches (they are found first); by default an overflow is repeated
        once with the size the call reports.  Returns (records, sums)."""
        t, n_sym = self._text(text)
        return _segment_host_call(self.L.acm_segment, "acm_segment", (self.handle, t.ctypes.data, n_sym), cost, gap_cost,
                                  int(capacity) if capacity is not None else max(1024, t.size // 64), capacity is not None)

    def scan_words(self, text, ranges=ASCII_WORD, flags="both", capacity=None):
        """acm_scan_words(): the whole-word matches of `text` in canonical order (see words_records).
        `capacity` must hold ALL matches (they are found first); by default an overflow is repeated
        once with the size the call reports."""
        t, n_sym = self._text(text)
        r, nr = _word_ranges(ranges, self.sym_size)
        return _records_host_call(self.L.acm_scan_words, "acm_scan_words", (self.handle, t.ctypes.data, n_sym, r.ctypes.data, nr, _word_flags(flags)),
                                  int(capacity) if capacity is not None else max(1024, t.size // 64), capacity is not None)

    def scan_chars(self, text, unit="codepoints", capacity=None):
        """acm_scan_chars(): the matches of the UTF-8 bytes `text` in canonical order and where each lies in code
        points ("codepoints") or UTF-16 code units ("utf16"): (records, char_start, char_len, edge), see
        chars_records.  `capacity` must hold ALL matches; by default an overflow is repeated once with the size the
        call reports."""
        t, n_sym = self._text(text)
        return _chars_host_call(self.L.acm_scan_chars, "acm_scan_chars", (self.handle, t.ctypes.data, n_sym, _chars_unit(unit)),
                                int(capacity) if capacity is not None else max(1024, t.size // 64), capacity is not None)

    def scan_str(self, s, unit="codepoints"):
        """The matches of the keywords (UTF-8 bytes) in the str `s`, in the indices of `s` itself: a structured array
        (start, stop, keyword_id, edge) in canonical order, s[start:stop] the match when edge is 0 -- "codepoints"
        for a Python str, "utf16" for the strings of Java, JavaScript and the Language Server Protocol.  edge != 0
        marks a match of bytes that begins or ends inside a character (include/acm_chars.h)."""
        if self.sym_size != 1:
            raise ValueError("scan_str needs a machine over bytes (sym_size 1), not %r" % (self.sym_size,))
        rec, start, length, edge = self.scan_chars(s.encode("utf-8"), unit)
        out = np.zeros(rec.size, STR_MATCH_DTYPE)
        out["start"], out["stop"], out["keyword_id"], out["edge"] = start, start + length, rec["keyword_id"], edge
        return out

    def context(self, text, before=0, after=0, merge=True, capacity=None, gather=True, out_capacity=None):
        """acm_context(): the matches of `text` with `before` symbols in front of and `after` behind each
        (see context_records), as a Snippets of numpy arrays whose `records` are the matches in canonical
        order.  `capacity` must hold ALL matches; by default each overflow is repeated once with the size
        the call reports."""
        t, n_sym = self._text(text)
        call = _context_scan_call(self.L.acm_context, (self.handle,), t, n_sym, (), before, after, _context_flags("symbols", merge))
        return _context_host_call(call, "acm_context", t, self.sym_size, int(capacity) if capacity is not None else max(1024, t.size // 64),
                                  capacity is None, gather, out_capacity)

    def scan_patterns(self, text, patternset, offsets=None, out_capacity=None):
        """acm_scan_patterns(): the matches of the patterns of `patternset` (see patterns_records) in `text`,
        or in every text of the buffer when `offsets` (n_texts + 1 entries) cuts it; by default an overflow is
        repeated once with the size the call reports."""
        return self._scan_set("acm_scan_patterns", text, _patternset(patternset), offsets, out_capacity, extra=())[0]

    def scan_chains(self, text, chainset, offsets=None, out_capacity=None):
        """acm_scan_chains(): the matches of the chains of `chainset` (see chains_records) in `text`, or in
        every text of the buffer when `offsets` (n_texts + 1 entries) cuts it; by default an overflow is
        repeated once with the size the call reports."""
        return self._scan_set("acm_scan_chains", text, _chainset(chainset), offsets, out_capacity, extra=())[0]

    def scan_near(self, text, nearset, offsets=None, out_capacity=None):
        """acm_scan_near(): the matches of the groups of `nearset` (see near_records) in `text`, or in every
        text of the buffer when `offsets` (n_texts + 1 entries) cuts it; by default an overflow is repeated
        once with the size the call reports."""
        return self._scan_set("acm_scan_near", text, _nearset(nearset), offsets, out_capacity, extra=())[0]

    def scan_approx(self, text, approxset, offsets=None, out_capacity=None):
        """acm_scan_approx(): (matches, dist) of the targets of `approxset` (see approx_records) in `text`, or in
        every text of the buffer when `offsets` (n_texts + 1 entries) cuts it; by default an overflow is repeated
        once with the size the call reports."""
        return self._scan_set("acm_scan_approx", text, approxset, offsets, out_capacity)

    def scan_edit(self, text, approxset, offsets=None, out_capacity=None):
        """acm_scan_edit(): (matches, dist) of the targets of `approxset` within edit distance k (see edit_records) in
        `text`, or in every text of the buffer when `offsets` cuts it; arguments as scan_approx()."""
        return self._scan_set("acm_scan_edit", text, approxset, offsets, out_capacity)

    def scan_templates(self, text, templateset, offsets=None, out_capacity=None):
        """acm_scan_templates(): (matches, dist) of the templates of `templateset` (a TemplateSet, see
        templates_records) in `text`, or in every text of the buffer when `offsets` cuts it; arguments as scan_approx()."""
        return self._scan_set("acm_scan_templates", text, templateset, offsets, out_capacity)

    def _scan_set(self, name, text, tset, offsets, out_capacity, extra=(np.uint32,)):
        """what the scans for the sets of a family share -- patterns and chains, and with a distance per match
        (`extra`) approx, edit and templates --: the machine-level C call `name`"""
        t, n_sym = self._text(text)
        off = np.ascontiguousarray(offsets, dtype=np.uint64) if offsets is not None else None
        return _matches_host_call(getattr(self.L, name), name, (self.handle, _ptr(t), n_sym, *_cut(off), *tset.args()), out_capacity, extra)

    def replace(self, text, replacements=None, fill=None, out_capacity=None):
        """acm_replace(): `text` with its leftmost-longest non-overlapping matches (select()) replaced:
        by `replacements`, a list with one entry per keyword in keyword_id order (`bytes` or arrays
        of symbols, an empty one deletes the match), or every symbol of every match by the ONE symbol
        `fill`.  Returns (the new text as an array of the machine's symbols, the number of matches
        replaced).  out_capacity (symbols): by default an output overflow is repeated once with the
        size the call reports."""
        return _replace_host_call(self.L.acm_replace, "acm_replace", self.handle, self._text(text)[0], self.sym_size, replacements, fill, out_capacity)

    def tokenize(self, texts_or_text, mode="run", gap_base=0, tok_of=None, token_capacity=None):
        """acm_tokenize(): the MaxMatch (greedy longest-match) tokens of one text (bytes or an array of
        symbols) or of a list of texts, each scanned from the root on its own, in ONE call: one token
        per selected match (id = tok_of[keyword_id], or the keyword id), and for the symbols no keyword
        covers by `mode` one token each ("symbol": gap_base + the symbol's value, 1- and 2-byte
        symbols), one token per run ("run": gap_base) or none ("drop").  Returns a Tokens of numpy
        arrays; `first` holds the row pointers of a list.  The call counts first and then fills."""
        if isinstance(texts_or_text, (list, tuple)):
            packed, off = self._pack_texts(texts_or_text)
        else:
            packed, off = self._pack_texts([texts_or_text])[0], None
        return _tokenize_host_call(self.L.acm_tokenize, "acm_tokenize", self.handle, packed, self.sym_size, off, mode, gap_base, tok_of, token_capacity)

    def grep(self, texts, invert=False, gather=True):
        """acm_grep(): `grep -F -f` over a list of texts (bytes or arrays of symbols), each scanned from
        the root on its own in ONE call.  Returns a Grepped of numpy arrays: hits per text, the ids of
        the texts with a match (invert: of those without one) and, with gather, those texts packed in
        `out` with their offsets."""
        packed, offsets = self._pack_texts(texts)
        return _grep_host_call(self.L.acm_grep, "acm_grep", self.handle, packed, self.sym_size, offsets, invert, gather, None)

    def grep_lines(self, buffer, delims=b"\n", runs=False, invert=False, gather=True):
        """acm_grep_lines(): `grep -F -f keywords file` on a raw buffer (bytes or an array of symbols):
        cut into texts at the delimiter symbols -- lines, or with runs words --, each text scanned from
        the root on its own, all in ONE call.  Returns a Grepped of numpy arrays that also carries the
        `offsets` the buffer was cut at and `n_texts`; a kept line keeps its delimiter."""
        if self.sym_size in _SYM_DTYPE:
            t = self._symbols(buffer).reshape(-1)
        else:
            t = np.frombuffer(bytes(buffer), dtype=np.uint8) if isinstance(buffer, (bytes, bytearray)) else np.ascontiguousarray(buffer).reshape(-1)
        d, nd = _delims(delims, self.sym_size)
        return _grep_lines_host_call(self.L.acm_grep_lines, "acm_grep_lines", self.handle, t, self.sym_size, d, nd, runs, invert, gather)

    def tally_batch(self, texts):
        """acm_tally_batch(): which keywords occur how often in which text of a list of texts (bytes or
        arrays of symbols), each scanned from the root on its own in ONE call.  Returns a TalliedBatch
        of numpy arrays: the text x keyword count matrix in CSR form."""
        packed, offsets = self._pack_texts(texts)
        return _tally_batch_host_call(self.L.acm_tally_batch, "acm_tally_batch", self.handle, packed, self.sym_size, offsets)

    def rules(self, texts, ruleset):
        """acm_rules(): which rules of `ruleset` (a RuleSet, or a list of rule()s) fire in which text of
        a list of texts, each scanned from the root on its own in ONE call.  Returns a Fired of numpy
        arrays: the text x rule matrix in CSR form."""
        packed, offsets = self._pack_texts(texts)
        return _rules_host_call(self.L.acm_rules, "acm_rules", self.handle, packed, self.sym_size, offsets, ruleset)

    def score(self, texts, model, k=0):
        """acm_score(): the kept scores of `model` (a ScoreModel, or a list of score_class()es) for every
        text of a list of texts, each scanned from the root on its own in ONE call, every text's best
        class and, with k > 0, every class's best k texts.  Returns a Scored of numpy arrays."""
        packed, offsets = self._pack_texts(texts)
        return _score_host_call(self.L.acm_score, "acm_score", self.handle, packed, self.sym_size, offsets, model, k)

    def index(self, texts, n_keywords=None, text_base=0):
        """acm_index(): the inverted index of a list of texts (bytes or arrays of symbols), each scanned
        from the root on its own in ONE call: which texts hold keyword k, and how often.  n_keywords
        (None: the machine's) may be larger for a dictionary that will grow; text ids start at
        text_base.  Returns an Indexed of numpy arrays."""
        packed, offsets = self._pack_texts(texts)
        nk = self.nb_keywords if n_keywords is None else int(n_keywords)
        return _index_host_call(self.L.acm_index, "acm_index", self.handle, packed, self.sym_size, offsets, nk, text_base)

    def cooccur(self, texts, flags=0, row_limit=0, n_keywords=None):
        """acm_cooccur(): the keyword co-occurrence matrix of a list of texts (bytes or arrays of symbols),
        each scanned from the root on its own in ONE call: which keywords occur together, and in how many
        texts (flags: ACM_COOCCUR_PRODUCT sums the products of the counts, ACM_COOCCUR_DIAGONAL keeps
        a == b; row_limit > 0 leaves out the texts with more keywords than that).  n_keywords (None: the
        machine's) may be larger for a dictionary that will grow.  Returns a Cooccurred of numpy arrays."""
        packed, offsets = self._pack_texts(texts)
        nk = self.nb_keywords if n_keywords is None else int(n_keywords)
        return _cooccur_host_call(self.L.acm_cooccur, "acm_cooccur", self.handle, packed, self.sym_size, offsets, nk, _cooccur_flags(flags), row_limit)


class Replaced:
    """What Plan.replace_records() and Plan.scan_replace() leave on the device: `out` (a uint8 tensor,
    the first out_symbols symbols are the new text when out_symbols <= out_capacity), out_symbols and
    count (Python ints, read after a synchronise), records (the selection: int64 [capacity, 2]),
    out_start (an int64 tensor, one entry per record, or None)."""

    def __init__(self, out, out_symbols, out_capacity, records, count, out_start):
        self.out, self.out_symbols, self.out_capacity = out, out_symbols, out_capacity
        self.records, self.count, self.out_start = records, count, out_start


class _DeviceSet(_Owner):
    """A set of a family compiled for a plan's device.  A subclass declares STEM (its C calls are
    acm_gpu_<STEM>_create, _info and _destroy), INFO (the struct _info fills), SIZE (the attribute that holds the
    number of its members, here and in its host description) and _host (what makes a host description of the
    caller's argument)."""
    _host = staticmethod(lambda description: description)

    def __init__(self, handle, size):
        self.h = handle
        setattr(self, self.SIZE, size)

    @classmethod
    def create(cls, plan, description):
        """acm_gpu_<STEM>_create(): the host description compiled and uploaded to the plan's device"""
        d = cls._host(description)
        name = "acm_gpu_%s_create" % cls.STEM
        h = C.c_void_p()
        _check(getattr(lib(), name)(plan.h, *d.args(), C.byref(h)), name)
        return cls(h, getattr(d, cls.SIZE))

    @classmethod
    @contextlib.contextmanager
    def for_call(cls, plan, given, sync=False):
        """The device set of one call: `given` itself when it is one, else its host description compiled for
        this call and closed behind it.  sync: the current stream is synchronised before such a set goes away,
        for the callers that queue work and return without reading a result."""
        if isinstance(given, cls):
            yield given
            return
        made = cls.create(plan, given)
        try:
            yield made
            if sync:
                import torch
                torch.cuda.current_stream().synchronize()
        finally:
            made.close()

    def info(self):
        """acm_gpu_<STEM>_info(): the figures of the set as a dict (the class says which)"""
        i = self.INFO()
        name = "acm_gpu_%s_info" % self.STEM
        _check(getattr(lib(), name)(self.h, C.byref(i)), name)
        return {n: int(getattr(i, n)) for n, _ in self.INFO._fields_}

    def close(self):
        if self.h:
            getattr(lib(), "acm_gpu_%s_destroy" % self.STEM)(self.h)
            self.h = None


class Rules(_DeviceSet):
    """A rule set on a plan's device (ACMRules): Plan.rules_create() makes one.  info(): rules, terms,
    always_rules, postings and the texts the set's evaluations sent through the fast and the wide form so far;
    waits for the device."""
    STEM, INFO, SIZE, _host = "rules", RulesInfo, "n_rules", staticmethod(_ruleset)


class Score(_DeviceSet):
    """A score model on a plan's device (ACMScore): Plan.score_create() makes one.  info(): classes, terms,
    postings, always_classes and the texts the model's evaluations sent through the fast and the wide form so
    far; waits for the device."""
    STEM, INFO, SIZE, _host = "score", ScoreInfo, "n_classes", staticmethod(_scoremodel)


class Patterns(_DeviceSet):
    """A pattern set on a plan's device (ACMPatterns): Plan.patterns_create() makes one.  info(): patterns,
    terms, anchor_keywords, longest and max_anchor_postings; n records give at most n * max_anchor_postings
    matches (MOST)."""
    STEM, INFO, SIZE, _host, MOST = "patterns", PatternsInfo, "n_patterns", staticmethod(_patternset), "max_anchor_postings"


class Chains(_DeviceSet):
    """A chain set on a plan's device (ACMChains): Plan.chains_create() makes one.  info(): chains, terms,
    max_terms, max_gap, max_postings and max_last_postings; n records give at most n * max_last_postings
    matches (MOST)."""
    STEM, INFO, SIZE, _host, MOST = "chains", ChainsInfo, "n_chains", staticmethod(_chainset), "max_last_postings"


class Near(_DeviceSet):
    """A NEAR group set on a plan's device (ACMNear): Plan.near() makes one.  info(): groups, terms, max_terms,
    max_width and max_postings; n records give at most n * max_postings matches (MOST)."""
    STEM, INFO, SIZE, _host, MOST = "near", NearInfo, "n_groups", staticmethod(_nearset), "max_postings"


class Approx(_DeviceSet):
    """A target set with mismatch budgets on a plan's device (ACMApprox): Plan.approx_create() makes one.
    info(): targets, terms, seed_keywords, longest, max_k and max_postings; n records give at most n *
    max_postings matches (the edit calls: times 2 * max_k + 1)."""
    STEM, INFO, SIZE = "approx", ApproxInfo, "n_targets"


class Templates(Approx):
    """A template set on a plan's device (ACMTemplates): Plan.templates_create() makes one.  info(): templates,
    terms, classes, seed_keywords, longest, max_k and max_postings; n records give at most n * max_postings
    matches."""
    STEM, INFO = "templates", TemplatesInfo


class Plan(_Owner):
    """Device-resident flattened automaton (ACMPlan).  Scans take torch CUDA tensors (device
    memory and streams are torch's; the kernels are this library's)."""

    def __init__(self, handle, sym_size):
        self.h = handle
        self.sym_size = sym_size
        info = PlanInfo()
        lib().acm_gpu_plan_info(handle, C.byref(info))
        self.info = info

    def close(self):
        if self.h:
            lib().acm_gpu_plan_destroy(self.h)
            self.h = None

    def update(self, machine):
        """acm_gpu_plan_update(): take over the keywords added to `machine` since this plan was made."""
        _check(lib().acm_gpu_plan_update(self.h, machine.handle), "acm_gpu_plan_update")
        lib().acm_gpu_plan_info(self.h, C.byref(self.info))

    def describe(self):
        i = self.info
        return {n: getattr(i, n) for n, _ in PlanInfo._fields_}

    @staticmethod
    def _stream():
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _text_args(self, text, n_symbols=None):
        """the checks of a device call on `text`; returns n_symbols, by default what the tensor holds"""
        assert text.is_cuda and text.is_contiguous()
        return text.numel() * text.element_size() // self.sym_size if n_symbols is None else n_symbols

    def _batch_args(self, text, offsets):
        """the checks of a device call on a batch -- `text` and its int64 `offsets`, n_texts + 1 of them --;
        returns (n_symbols, n_texts)"""
        import torch
        assert text.is_cuda and text.is_contiguous() and offsets.is_cuda and offsets.is_contiguous() and offsets.dtype == torch.int64
        n_texts = offsets.numel() - 1
        assert n_texts >= 0
        return text.numel() * text.element_size() // self.sym_size, n_texts

    @staticmethod
    def _windows(window, capacity, pair_capacity=None):
        """(window, capacity, pair_capacity) of the tally in front of a call, by default 16 Mi symbols a window,
        1 Mi records a window and as many pairs as records"""
        window = int(window) if window is not None else 1 << 24
        capacity = int(capacity) if capacity is not None else 1 << 20
        return window, capacity, int(pair_capacity) if pair_capacity is not None else capacity

    @staticmethod
    def _records_out(records, count, capacity, n_symbols, dev):
        """(records, count) of a scan that leaves both on the device: the caller's tensors, or new ones -- `capacity`
        records, by default one for every 256 symbols and 4096 at the least, and a zeroed count"""
        import torch
        if records is None:
            cap = int(capacity) if capacity is not None else max(4096, n_symbols // 256)
            records = torch.empty((cap, 2), dtype=torch.int64, device=dev)
        return records, count if count is not None else _i64(1, dev)

    @staticmethod
    def _records_room(records, capacity, n_symbols, dev):
        """(records, capacity) of a scan into records of the call's own: the caller's tensor, or a new one of
        `capacity` records, by default one for every 256 symbols and 4096 at the least"""
        import torch
        if records is not None:
            return records, records.shape[0] if capacity is None else int(capacity)
        cap = int(capacity) if capacity is not None else max(4096, n_symbols // 256)
        return torch.empty((max(cap, 1), 2), dtype=torch.int64, device=dev), cap

    def scan(self, text, n_symbols=None, emit_from=0, pos_base=0, capacity=None, records=None, count=None):
        """Unsorted scan of a device tensor (uint8 storage of n_symbols * sym_size bytes, or a
        tensor of the symbol dtype).  Returns (records u64[capacity, 2] tensor, count tensor).
        Asynchronous on the current stream."""
        import torch
        assert text.is_cuda and text.is_contiguous()
        if n_symbols is None:
            n_symbols = text.numel() * text.element_size() // self.sym_size
        if records is None:
            cap = int(capacity) if capacity is not None else max(4096, n_symbols // 256)
            records = torch.empty((cap, 2), dtype=torch.int64, device=text.device)
        if count is None:
            count = torch.zeros(1, dtype=torch.int64, device=text.device)
        _check(lib().acm_gpu_scan_device(self.h, text.data_ptr(), n_symbols, emit_from, pos_base, records.data_ptr(),
                                         records.shape[0], count.data_ptr(), self._stream()), "acm_gpu_scan_device")
        return records, count

    def scan_ordered(self, text, n_symbols=None, emit_from=0, pos_base=0, capacity=None, records=None, count=None, tmp=None):
        """acm_gpu_scan_ordered_device(): scan + canonical order, queued on the current stream with
        no host round trip in between (the order passes read the count on the device).  Returns
        (records, count, tmp); records[:count] is in canonical order when count <= capacity."""
        import torch
        assert text.is_cuda and text.is_contiguous()
        if n_symbols is None:
            n_symbols = text.numel() * text.element_size() // self.sym_size
        if records is None:
            cap = int(capacity) if capacity is not None else max(4096, n_symbols // 256)
            records = torch.empty((cap, 2), dtype=torch.int64, device=text.device)
        if count is None:
            count = torch.zeros(1, dtype=torch.int64, device=text.device)
        tb = lib().acm_gpu_scan_ordered_tmp_bytes(self.h, records.shape[0], n_symbols)
        if tmp is None or tmp.numel() < tb:
            tmp = torch.empty(tb, dtype=torch.uint8, device=text.device)
        _check(lib().acm_gpu_scan_ordered_device(self.h, text.data_ptr(), n_symbols, emit_from, pos_base, records.data_ptr(),
                                                 records.shape[0], count.data_ptr(), tmp.data_ptr(), tmp.numel(), self._stream()),
               "acm_gpu_scan_ordered_device")
        return records, count, tmp

    def count(self, text, n_symbols=None, emit_from=0, count=None):
        import torch
        if n_symbols is None:
            n_symbols = text.numel() * text.element_size() // self.sym_size
        if count is None:
            count = torch.zeros(1, dtype=torch.int64, device=text.device)
        _check(lib().acm_gpu_count_device(self.h, text.data_ptr(), n_symbols, emit_from, count.data_ptr(),
                                          self._stream()), "acm_gpu_count_device")
        return count

    def sort(self, records, n, pos_lo=None, span=None):
        """Canonical order (end_pos asc, length desc) of the first n records, in place.  With the
        range of their positions given ([pos_lo, pos_lo + span): what a scan of `span` symbols with
        pos_base = pos_lo leaves) acm_gpu_order_records_device orders them by position buckets and
        LDS sorts; without, acm_gpu_sort_records_device radix-sorts them."""
        import torch
        if n <= 1:
            return records
        if pos_lo is None or span is None:
            tb = lib().acm_gpu_sort_tmp_bytes(n)
            tmp = torch.empty(tb, dtype=torch.uint8, device=records.device)
            _check(lib().acm_gpu_sort_records_device(self.h, records.data_ptr(), n, tmp.data_ptr(), tb, self._stream()),
                   "acm_gpu_sort_records_device")
            return records
        tb = lib().acm_gpu_order_tmp_bytes(self.h, n, span)
        tmp = torch.empty(tb, dtype=torch.uint8, device=records.device)
        _check(lib().acm_gpu_order_records_device(self.h, records.data_ptr(), n, pos_lo, span, tmp.data_ptr(), tb, self._stream()),
               "acm_gpu_order_records_device")
        return records

    def scan_sorted(self, text, n_symbols=None, emit_from=0, pos_base=0, capacity=None, fused=True):
        """Scan + canonical order; grows the record buffer when it overflowed (nothing is dropped).
        fused: acm_gpu_scan_ordered_device (one call), else acm_gpu_scan_device, the count read
        back, acm_gpu_order_records_device.  Returns a numpy structured array (RECORD_DTYPE)."""
        cap = capacity
        while True:
            if fused:
                rec, cnt, _ = self.scan_ordered(text, n_symbols, emit_from, pos_base, cap)
            else:
                rec, cnt = self.scan(text, n_symbols, emit_from, pos_base, cap)
            n = int(cnt.item())
            if n > rec.shape[0]:
                cap = n
                continue
            if not fused:
                ns = n_symbols if n_symbols is not None else text.numel() * text.element_size() // self.sym_size
                self.sort(rec, n, pos_base, ns)
            self.status()
            return np.frombuffer(rec[:n].cpu().numpy().tobytes(), dtype=RECORD_DTYPE).copy()

    def scan_host(self, text, emit_from=0, pos_base=0, capacity=None):
        """acm_gpu_scan_host(): numpy in, numpy out, through the C ABI only (no torch)."""
        t = np.ascontiguousarray(text)
        n_sym = t.size * t.itemsize // self.sym_size
        return _records_host_call(lib().acm_gpu_scan_host, "acm_gpu_scan_host", (self.h, t.ctypes.data, n_sym, emit_from, pos_base),
                                  int(capacity) if capacity is not None else max(1024, n_sym // 64), capacity is not None, repeats=None)

    def scan_batch(self, text, offsets, capacity=None):
        """acm_gpu_scan_batch_device(): `text` is a device tensor holding the texts of a batch side
        by side, `offsets` an int64 device tensor of n_texts + 1 entries (text t = symbols
        [offsets[t], offsets[t + 1])).  Every text is scanned from the root on its own.  Returns
        numpy arrays (records, text_id, first): the records in canonical order with end_pos = the
        index in `text`, the text of each, and first[t] .. first[t + 1] = the records of text t.
        capacity must hold the matches of the whole buffer: by default Plan.count() says how many
        there are, and an overflow is repeated once with the size the call reports."""
        n_symbols, n_texts = self._batch_args(text, offsets)

        def launch(records, text_id, first, cap, count):
            tmp = _scratch(lib().acm_gpu_scan_batch_tmp_bytes(self.h, cap, n_symbols, n_texts), text.device)
            _check(lib().acm_gpu_scan_batch_device(self.h, text.data_ptr(), n_symbols, offsets.data_ptr(), n_texts, records.data_ptr(),
                                                   text_id.data_ptr(), first.data_ptr(), cap, count.data_ptr(), tmp.data_ptr(), tmp.numel(),
                                                   self._stream()), "acm_gpu_scan_batch_device")
        return self._batch_records_device(launch, "acm_gpu_scan_batch_device", text.device, n_texts,
                                          int(capacity) if capacity is not None else max(int(self.count(text).item()), 1))

    def _batch_records_device(self, launch, what, dev, n_texts, cap):
        """what scan_batch() and Flows.scan() share: launch(records, text_id, first, cap, count) into tensors of
        the call's own, repeated once with the count when that is above cap, then the plan's status and the
        three as numpy arrays (records, text_id, first)"""
        import torch

        def run(cap):
            records = torch.empty((max(cap, 1), 2), dtype=torch.int64, device=dev)
            text_id = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
            first, count = _i64(n_texts + 1, dev), _i64(1, dev)
            launch(records, text_id, first, cap, count)
            return int(count.item()), (records, text_id, first)
        n, (records, text_id, first) = _device_room_call(run, what, cap)
        self.status()
        return (np.frombuffer(records[:n].cpu().numpy().tobytes(), dtype=RECORD_DTYPE).copy(),
                text_id[:n].cpu().numpy().view(np.uint32).copy(), first.cpu().numpy().view(np.uint64).copy())

    def scan_batch_host(self, text, offsets, capacity=None):
        """acm_gpu_scan_batch_host(): the same from host arrays, through the C ABI only (no torch)."""
        t = np.ascontiguousarray(text)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        assert off.size >= 1, "offsets has n_texts + 1 entries"
        return _batch_records_host_call(lib().acm_gpu_scan_batch_host, "acm_gpu_scan_batch_host", (self.h, t.ctypes.data, off.ctypes.data, off.size - 1),
                                        off.size - 1, int(capacity) if capacity is not None else max(1024, t.size * t.itemsize // self.sym_size // 64))

    def scan_anchored(self, text, offsets, mode="prefixes", capacity=None, records=None, text_id=None, first=None, count=None, tmp=None):
        """acm_gpu_scan_anchored_device(): `text` and `offsets` as Plan.scan_batch takes them.  The
        keywords every text begins with (mode "prefixes"), the longest of them ("longest") or the
        keyword that spells the whole text ("whole"), found by a walk from the root with no scan.
        Queued on the current stream; returns device tensors (records int64 [capacity, 2], text_id
        int32, first int64 [n_texts + 1], count int64 [1], tmp).  capacity holds the anchored records
        only: by default n_texts, which "longest" and "whole" cannot exceed; count > capacity says
        what "prefixes" needs, and first is complete either way."""
        import torch
        n_symbols, n_texts = self._batch_args(text, offsets)
        dev = text.device
        if records is None:
            records = torch.empty((max(int(capacity) if capacity is not None else n_texts, 1), 2), dtype=torch.int64, device=dev)
        cap = records.shape[0] if capacity is None else int(capacity)
        if text_id is None:
            text_id = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        if first is None:
            first = _i64(n_texts + 1, dev)
        if count is None:
            count = _i64(1, dev)
        tmp = _scratch(lib().acm_gpu_scan_anchored_tmp_bytes(self.h, n_texts), dev, tmp)
        _check(lib().acm_gpu_scan_anchored_device(self.h, text.data_ptr(), n_symbols, offsets.data_ptr(), n_texts, _anchored_mode(mode),
                                                  records.data_ptr(), text_id.data_ptr(), first.data_ptr(), cap, count.data_ptr(), tmp.data_ptr(),
                                                  tmp.numel(), self._stream()), "acm_gpu_scan_anchored_device")
        return records, text_id, first, count, tmp

    def lookup(self, text, offsets, whole_id=True, prefix_id=True, prefix_len=True, tmp=None):
        """acm_gpu_lookup_device(): one answer per text of a batch on the device, queued on the current
        stream -- int32 device tensors (whole_id, prefix_id, prefix_len) of n_texts entries: the id
        of the keyword that spells the whole text (a column's dictionary code), the id and the
        length of the longest keyword the text begins with; -1 (ACM_LOOKUP_NONE) / 0 where there is
        none.  An output given as False is not computed (None comes back); a tensor is written in place."""
        import torch
        n_symbols, n_texts = self._batch_args(text, offsets)
        outs = [torch.empty(max(n_texts, 1), dtype=torch.int32, device=text.device) if o is True else (None if o is False or o is None else o)
                for o in (whole_id, prefix_id, prefix_len)]
        tmp = _scratch(lib().acm_gpu_lookup_tmp_bytes(self.h, n_texts), text.device, tmp)
        _check(lib().acm_gpu_lookup_device(self.h, text.data_ptr(), n_symbols, offsets.data_ptr(), n_texts, *[_opt(o) for o in outs], tmp.data_ptr(),
                                           tmp.numel(), self._stream()), "acm_gpu_lookup_device")
        return tuple(o[:n_texts] if o is not None else None for o in outs)

    def scan_anchored_host(self, text, offsets, mode="prefixes", capacity=None):
        """acm_gpu_scan_anchored_host(): the same from host arrays, through the C ABI only (no torch):
        numpy arrays (records, text_id, first)."""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        assert off.size >= 1, "offsets has n_texts + 1 entries"
        return _anchored_host_call(lib().acm_gpu_scan_anchored_host, "acm_gpu_scan_anchored_host", self.h, np.ascontiguousarray(text), off, mode,
                                   capacity)

    def lookup_host(self, text, offsets):
        """acm_gpu_lookup_host(): numpy in, (whole_id, prefix_id, prefix_len) out, through the C ABI only."""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        assert off.size >= 1, "offsets has n_texts + 1 entries"
        return _lookup_host_call(lib().acm_gpu_lookup_host, "acm_gpu_lookup_host", self.h, np.ascontiguousarray(text), off)

    @property
    def tally_form(self):
        """acm_gpu_tally_form(): 1 = the plan's tally kernel counts in LDS, 2 = with global atomics."""
        return int(lib().acm_gpu_tally_form(self.h))

    @property
    def tally_keywords(self):
        """acm_gpu_tally_keywords(): the counters a tally of this plan needs."""
        return int(lib().acm_gpu_tally_keywords(self.h))

    def tally(self, text, n_symbols=None, emit_from=0, tally=None, window=None, capacity=None):
        """acm_gpu_tally_device(): per-keyword match counts of a device tensor; no record leaves the
        device.  `tally` (an int64 device tensor with at least tally_keywords entries; None: a zeroed
        one) is ADDED TO.  `window` (symbols, a multiple of 16) and `capacity` (records per window)
        default to 16 Mi symbols and 1 Mi records.  Returns (tally, total, need): need > capacity says
        that a window overflowed -- tally is untouched and total is 0 then, and a capacity of `need`
        suffices for the same window.  Synchronises to read total and need."""
        import torch
        n_symbols = self._text_args(text, n_symbols)
        window, capacity, _ = self._windows(window, capacity)
        if tally is None:
            tally = _i64(max(self.tally_keywords, 1), text.device)
        assert tally.is_cuda and tally.is_contiguous() and tally.dtype == torch.int64
        out = _i64(2, text.device)
        tmp = _scratch(lib().acm_gpu_tally_tmp_bytes(self.h, window, capacity), text.device)
        _check(lib().acm_gpu_tally_device(self.h, text.data_ptr(), n_symbols, emit_from, tally.data_ptr(), tally.numel(), window, capacity,
                                          out.data_ptr(), out.data_ptr() + 8, tmp.data_ptr(), tmp.numel(), self._stream()),
               "acm_gpu_tally_device")
        total, need = (int(x) for x in out.cpu())
        return tally, total, need

    def tally_host(self, text):
        """acm_gpu_tally_host(): numpy in, (np.uint64 counters, total) out, through the C ABI only (no
        torch).  The call sizes its windows itself and never overflows."""
        t = np.ascontiguousarray(text)
        tally = np.zeros(max(self.tally_keywords, 1), dtype=np.uint64)
        total = C.c_uint64(0)
        _check(lib().acm_gpu_tally_host(self.h, t.ctypes.data, t.size * t.itemsize // self.sym_size, tally.ctypes.data, tally.size,
                                        C.byref(total)), "acm_gpu_tally_host")
        return tally, int(total.value)

    def grep(self, text, offsets, invert=False, window=None, capacity=None, gather=True, out=None, out_capacity=None):
        """acm_gpu_grep_device(): `grep -F -f` over a batch on the device.  `text` is a device tensor
        holding the texts side by side, `offsets` an int64 device tensor of n_texts + 1 entries.  No
        record leaves the device.  `window` (symbols, a multiple of 16) and `capacity` (records per
        window) default to 16 Mi symbols and 1 Mi records.  With gather the kept texts are packed into
        `out` (None: a new uint8 tensor with room for out_capacity symbols, by default for the whole
        buffer; it must not overlap `text`).  Returns a Grepped of device tensors; synchronises to
        read its four numbers."""
        import torch
        n_symbols, n_texts = self._batch_args(text, offsets)
        window, capacity, _ = self._windows(window, capacity)
        dev = text.device
        hits = _i64(max(n_texts, 1), dev)
        kept = torch.zeros(max(n_texts, 1), dtype=torch.int32, device=dev)
        out_off = _i64(n_texts + 1, dev)
        res = _i64(4, dev)                                                       # n_kept, total, need, out_symbols
        out, out_capacity = self._gather_room(dev, gather, out, out_capacity, n_symbols)
        tmp = _scratch(lib().acm_gpu_grep_tmp_bytes(self.h, window, capacity, n_symbols, n_texts), dev)
        _check(lib().acm_gpu_grep_device(self.h, text.data_ptr(), n_symbols, offsets.data_ptr(), n_texts,
                                         ACM_GREP_INVERT if invert else ACM_GREP_MATCHING, window, capacity, hits.data_ptr(), kept.data_ptr(),
                                         res.data_ptr(), res.data_ptr() + 8, res.data_ptr() + 16, _opt(out), out_capacity, out_off.data_ptr(),
                                         res.data_ptr() + 24 if gather else None, tmp.data_ptr(), tmp.numel(), self._stream()), "acm_gpu_grep_device")
        n_kept, total, need, out_symbols = (int(x) for x in res.cpu())
        if not gather:
            out_symbols = int(out_off[n_kept].item()) if need <= capacity else 0
        return Grepped(hits[:n_texts], kept, n_kept, total, need, out, out_off, out_symbols, out_capacity)

    def _gather_room(self, dev, gather, out, out_capacity, n_symbols):
        """(out, out_capacity) of a call that packs symbols into `out` when `gather`: the caller's tensor, or a new
        uint8 one with room for out_capacity symbols, by default for the whole buffer; (None, 0) without"""
        import torch
        if not gather:
            return None, 0
        if out_capacity is None:
            out_capacity = out.numel() * out.element_size() // self.sym_size if out is not None else n_symbols
        if out is None:
            out = torch.empty(max(int(out_capacity) * self.sym_size, 16), dtype=torch.uint8, device=dev)
        assert out.is_cuda and out.is_contiguous() and out.numel() * out.element_size() >= int(out_capacity) * self.sym_size
        return out, int(out_capacity)

    def grep_host(self, text, offsets, invert=False, gather=True, out_capacity=None):
        """acm_gpu_grep_host(): the same from host arrays, through the C ABI only (no torch).  The call
        sizes its windows itself and never reports a record overflow.  Returns a Grepped of numpy arrays."""
        t = np.ascontiguousarray(text)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        assert off.size >= 1, "offsets has n_texts + 1 entries"
        return _grep_host_call(lib().acm_gpu_grep_host, "acm_gpu_grep_host", self.h, t, self.sym_size, off, invert, gather, out_capacity)

    def split(self, text, delims=b"\n", runs=False, capacity=None):
        """acm_gpu_split_device(): the offsets of the texts a device buffer holds between its delimiter
        symbols -- lines, or with runs words (a text is a word and the run of delimiters behind it); an
        unterminated last text counts.  `text` is a device tensor of symbols, `delims` up to 16 symbols
        (bytes: one symbol per byte).  Returns the int64 device tensor offsets[: n_texts + 1], which
        Plan.grep, Plan.scan_batch, Plan.tally_batch and Flows take as it is.  Without `capacity` the
        texts are counted first (one synchronise) and the tensor is sized by the count; with it the
        call raises ACM_GPU_E_OVERFLOW, the count needed in its `need`, when there are more texts."""
        n_symbols = self._text_args(text)
        d, nd = _delims(delims, self.sym_size)
        flags = ACM_SPLIT_RUNS if runs else ACM_SPLIT_EVERY
        dev = text.device
        tmp = _scratch(lib().acm_gpu_split_tmp_bytes(self.h, n_symbols), dev)
        count = _i64(1, dev)

        def call(off, cap):
            _check(lib().acm_gpu_split_device(self.h, text.data_ptr(), n_symbols, d.ctypes.data, nd, flags, _opt(off), cap, count.data_ptr(),
                                              tmp.data_ptr(), tmp.numel(), self._stream()), "acm_gpu_split_device")
        if capacity is None:
            call(None, 0)
            capacity = int(count.item())
        off = _i64(int(capacity) + 1, dev)
        call(off, int(capacity))
        n = int(count.item())
        if n > int(capacity):
            e = ACMError(ACM_GPU_E_OVERFLOW, "acm_gpu_split_device: %d texts, room for %d" % (n, int(capacity)))
            e.need = n
            raise e
        return off[:n + 1]

    def split_host(self, text, delims=b"\n", runs=False, capacity=None):
        """acm_gpu_split_host(): the same from a host array, through the C ABI only (no torch).  Returns
        the n_texts + 1 offsets as a numpy uint64 array; with `capacity`, raises on more texts as split()."""
        t = np.ascontiguousarray(text)
        n_symbols = t.size * t.itemsize // self.sym_size
        d, nd = _delims(delims, self.sym_size)
        flags = ACM_SPLIT_RUNS if runs else ACM_SPLIT_EVERY
        n = C.c_uint64(0)
        tp = t.ctypes.data if t.size else None
        if capacity is None:
            _check(lib().acm_gpu_split_host(self.h, tp, n_symbols, d.ctypes.data, nd, flags, None, 0, C.byref(n)), "acm_gpu_split_host")
            capacity = int(n.value)
        off = np.zeros(int(capacity) + 1, np.uint64)
        rc = lib().acm_gpu_split_host(self.h, tp, n_symbols, d.ctypes.data, nd, flags, off.ctypes.data, int(capacity), C.byref(n))
        if rc == ACM_GPU_E_OVERFLOW:
            e = ACMError(rc, "acm_gpu_split_host: %d texts, room for %d" % (n.value, int(capacity)))
            e.need = int(n.value)
            raise e
        _check(rc, "acm_gpu_split_host")
        return off[:int(n.value) + 1]

    def grep_lines_host(self, text, delims=b"\n", runs=False, invert=False, gather=True):
        """acm_gpu_grep_lines_host(): `grep -F -f` on a raw buffer in host memory: uploaded once, cut
        into texts on the device, then grep as grep_host() runs it.  Returns a Grepped of numpy arrays
        that also carries `offsets` and `n_texts`."""
        t = np.ascontiguousarray(text).reshape(-1)
        d, nd = _delims(delims, self.sym_size)
        return _grep_lines_host_call(lib().acm_gpu_grep_lines_host, "acm_gpu_grep_lines_host", self.h, t, self.sym_size, d, nd, runs, invert, gather)

    def tally_batch(self, text, offsets, window=None, capacity=None, pair_capacity=None):
        """acm_gpu_tally_batch_device(): the text x keyword count matrix of a batch on the device, in
        CSR form.  `text` is a device tensor holding the texts side by side, `offsets` an int64 device
        tensor of n_texts + 1 entries.  No record leaves the device.  `window` (symbols, a multiple of
        16) and `capacity` (records per window) default to 16 Mi symbols and 1 Mi records,
        `pair_capacity` (the room of col and val) to `capacity`.  Returns a TalliedBatch of device
        tensors; synchronises to read its four numbers."""
        import torch
        n_symbols, n_texts = self._batch_args(text, offsets)
        window, capacity, pair_capacity = self._windows(window, capacity, pair_capacity)
        dev = text.device
        row_ptr = _i64(n_texts + 1, dev)
        col = torch.zeros(max(pair_capacity, 1), dtype=torch.int32, device=dev)
        val = _i64(max(pair_capacity, 1), dev)
        res = _i64(4, dev)                                                       # nnz, total, need, need_pairs
        tmp = _scratch(lib().acm_gpu_tally_batch_tmp_bytes(self.h, window, capacity, pair_capacity, n_symbols, n_texts), dev)
        _check(lib().acm_gpu_tally_batch_device(self.h, text.data_ptr(), n_symbols, offsets.data_ptr(), n_texts, window, capacity, pair_capacity,
                                                row_ptr.data_ptr(), col.data_ptr(), val.data_ptr(), res.data_ptr(), res.data_ptr() + 8,
                                                res.data_ptr() + 16, res.data_ptr() + 24, tmp.data_ptr(), tmp.numel(), self._stream()),
               "acm_gpu_tally_batch_device")
        nnz, total, need, need_pairs = (int(x) for x in res.cpu())
        return TalliedBatch(row_ptr, col, val, nnz, total, need, need_pairs)

    def tally_batch_host(self, text, offsets):
        """acm_gpu_tally_batch_host(): the same from host arrays, through the C ABI only (no torch).
        The call sizes its windows and its pair room itself.  Returns a TalliedBatch of numpy arrays."""
        t = np.ascontiguousarray(text)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        assert off.size >= 1, "offsets has n_texts + 1 entries"
        return _tally_batch_host_call(lib().acm_gpu_tally_batch_host, "acm_gpu_tally_batch_host", self.h, t, self.sym_size, off)

    def rules_create(self, ruleset):
        """acm_gpu_rules_create(): `ruleset` (a RuleSet, or a list of rule()s) compiled and uploaded to
        this plan's device.  Returns a Rules; it stays valid across update()."""
        return Rules.create(self, ruleset)

    def _fired_outputs(self, dev, n_texts, fired_capacity):
        import torch
        fired = torch.zeros(max(fired_capacity, 1), dtype=torch.int32, device=dev) if fired_capacity else None
        return _i64(n_texts + 1, dev), fired

    @staticmethod
    def _matrix_args(tallied):
        """the checks of a device call on a count matrix (a TalliedBatch of device tensors); returns (row_ptr, col,
        val, n_texts)"""
        import torch
        row_ptr, col, val = tallied.row_ptr, tallied.col, tallied.val
        assert row_ptr.is_cuda and row_ptr.is_contiguous() and row_ptr.dtype == torch.int64
        assert col.is_contiguous() and col.dtype == torch.int32 and val.is_contiguous() and val.dtype == torch.int64
        n_texts = row_ptr.numel() - 1
        assert n_texts >= 0
        return row_ptr, col, val, n_texts

    def rules(self, text, offsets, rules, window=None, capacity=None, pair_capacity=None, fired_capacity=None):
        """acm_gpu_rules_device(): which rules fire in which text of a batch, on the device: the tally
        of tally_batch() (same `text`, `offsets`, `window`, `capacity`, `pair_capacity`) and the
        evaluation behind it in one call; neither a record nor the count matrix leaves the device.
        `rules` is a Rules from rules_create() (or a RuleSet / a list of rule()s, compiled for this
        call).  fired_capacity: the room of `fired` (0: count only; None: counted first, then sized by
        the count).  Returns a Fired of device tensors; synchronises to read its four numbers."""
        n_symbols, n_texts = self._batch_args(text, offsets)
        window, capacity, pair_capacity = self._windows(window, capacity, pair_capacity)
        dev = text.device
        with Rules.for_call(self, rules) as R:
            res = _i64(4, dev)                                                   # n_fired, total, need, need_pairs
            tmp = _scratch(lib().acm_gpu_rules_tmp_bytes(self.h, R.h, window, capacity, pair_capacity, n_symbols, n_texts), dev)

            def call(cap):
                fired_ptr, fired = self._fired_outputs(dev, n_texts, cap)
                _check(lib().acm_gpu_rules_device(self.h, R.h, text.data_ptr(), n_symbols, offsets.data_ptr(), n_texts, window, capacity, pair_capacity,
                                                  fired_ptr.data_ptr(), _opt(fired), cap, res.data_ptr(), res.data_ptr() + 8,
                                                  res.data_ptr() + 16, res.data_ptr() + 24, tmp.data_ptr(), tmp.numel(), self._stream()),
                       "acm_gpu_rules_device")
                n_fired, total, need, need_pairs = (int(x) for x in res.cpu())
                return Fired(fired_ptr, fired, n_fired, total, need, need_pairs, cap)
            return _counted(call, fired_capacity, "n_fired")

    def rules_matrix(self, tallied, rules, fired_capacity=None):
        """acm_gpu_rules_matrix_device(): the same for a count matrix that lies on the device: `tallied`
        is a TalliedBatch of device tensors, tally_batch()'s or the caller's own (row_ptr int64 with
        n_texts + 1 entries, col int32, val int64).  Returns a Fired of device tensors (total, need and
        need_pairs None); synchronises to read n_fired."""
        row_ptr, col, val, n_texts = self._matrix_args(tallied)
        dev = row_ptr.device
        with Rules.for_call(self, rules) as R:
            res = _i64(1, dev)
            tmp = _scratch(lib().acm_gpu_rules_matrix_tmp_bytes(self.h, R.h, n_texts), dev)

            def call(cap):
                fired_ptr, fired = self._fired_outputs(dev, n_texts, cap)
                _check(lib().acm_gpu_rules_matrix_device(self.h, R.h, row_ptr.data_ptr(), col.data_ptr(), val.data_ptr(), n_texts, fired_ptr.data_ptr(),
                                                         _opt(fired), cap, res.data_ptr(), tmp.data_ptr(), tmp.numel(), self._stream()),
                       "acm_gpu_rules_matrix_device")
                return Fired(fired_ptr, fired, int(res.item()), fired_capacity=cap)
            return _counted(call, fired_capacity, "n_fired")

    def rules_host(self, text, offsets, ruleset):
        """acm_gpu_rules_host(): the same as rules() from host arrays, through the C ABI only (no torch).
        The call sizes its windows and its pair room itself.  Returns a Fired of numpy arrays."""
        t = np.ascontiguousarray(text)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        assert off.size >= 1, "offsets has n_texts + 1 entries"
        return _rules_host_call(lib().acm_gpu_rules_host, "acm_gpu_rules_host", self.h, t, self.sym_size, off, ruleset)

    def score_create(self, model):
        """acm_gpu_score_create(): `model` (a ScoreModel, or a list of score_class()es) compiled and
        uploaded to this plan's device.  Returns a Score; it stays valid across update()."""
        return Score.create(self, model)

    def _kept_outputs(self, dev, n_texts, kept_capacity):
        import torch
        kept_ptr = _i64(n_texts + 1, dev)
        kept_class = torch.zeros(kept_capacity, dtype=torch.int32, device=dev) if kept_capacity else None
        kept_score = _i64(kept_capacity, dev) if kept_capacity else None
        best = torch.full((max(n_texts, 1),), -1, dtype=torch.int32, device=dev)[:n_texts] if kept_capacity else None
        return kept_ptr, kept_class, kept_score, best

    def _top_outputs(self, dev, n_classes, k):
        import torch
        return (torch.zeros(max(n_classes, 1), dtype=torch.int64, device=dev)[:n_classes],
                torch.zeros(max(n_classes, 1), dtype=torch.int32, device=dev)[:n_classes],
                torch.zeros((max(n_classes, 1), max(k, 1)), dtype=torch.int32, device=dev)[:n_classes, :k],
                torch.zeros((max(n_classes, 1), max(k, 1)), dtype=torch.int64, device=dev)[:n_classes, :k])

    def score(self, text, offsets, model, k=0, window=None, capacity=None, pair_capacity=None, kept_capacity=None):
        """acm_gpu_score_device(): the kept scores of every text of a batch, every text's best class and,
        with k > 0, every class's best k texts, on the device: the tally of tally_batch() (same `text`,
        `offsets`, `window`, `capacity`, `pair_capacity`), the evaluation and the ranking in one call.
        `model` is a Score from score_create() (or a ScoreModel / a list of score_class()es, compiled for
        this call).  kept_capacity: the room of the kept arrays (0: count only; None: counted first, then
        sized by the count).  Returns a Scored of device tensors; synchronises to read its four numbers."""
        n_symbols, n_texts = self._batch_args(text, offsets)
        window, capacity, pair_capacity = self._windows(window, capacity, pair_capacity)
        k = int(k)
        dev = text.device
        with Score.for_call(self, model) as S:
            res = _i64(4, dev)                                                   # n_kept, total, need, need_pairs

            def call(cap):
                tmp = _scratch(lib().acm_gpu_score_tmp_bytes(self.h, S.h, window, capacity, pair_capacity, n_symbols, n_texts, cap, k), dev)
                kept_ptr, kept_class, kept_score, best = self._kept_outputs(dev, n_texts, cap)
                hits, top_n, top_text, top_score = self._top_outputs(dev, S.n_classes, k) if k and cap else (None, None, None, None)
                p = _opt_full
                _check(lib().acm_gpu_score_device(self.h, S.h, text.data_ptr(), n_symbols, offsets.data_ptr(), n_texts, window, capacity, pair_capacity,
                                                  kept_ptr.data_ptr(), p(kept_class), p(kept_score), cap, res.data_ptr(), p(best),
                                                  k if hits is not None else 0, p(hits), p(top_n), p(top_text), p(top_score), res.data_ptr() + 8,
                                                  res.data_ptr() + 16, res.data_ptr() + 24, tmp.data_ptr(), tmp.numel(), self._stream()),
                       "acm_gpu_score_device")
                n_kept, total, need, need_pairs = (int(x) for x in res.cpu())
                return Scored(kept_ptr, kept_class, kept_score, n_kept, best, hits, top_n, top_text, top_score, total, need, need_pairs, cap)
            return _counted(call, kept_capacity, "n_kept")

    def score_matrix(self, tallied, model, kept_capacity=None):
        """acm_gpu_score_matrix_device(): the evaluation for a count matrix that lies on the device:
        `tallied` is a TalliedBatch of device tensors, tally_batch()'s or the caller's own (row_ptr int64
        with n_texts + 1 entries, col int32, val int64).  Returns a Scored of device tensors (no top
        arrays: score_top(); total, need and need_pairs None); synchronises to read n_kept."""
        row_ptr, col, val, n_texts = self._matrix_args(tallied)
        dev = row_ptr.device
        with Score.for_call(self, model) as S:
            res = _i64(1, dev)
            tmp = _scratch(lib().acm_gpu_score_matrix_tmp_bytes(self.h, S.h, n_texts), dev)

            def call(cap):
                kept_ptr, kept_class, kept_score, best = self._kept_outputs(dev, n_texts, cap)
                _check(lib().acm_gpu_score_matrix_device(self.h, S.h, row_ptr.data_ptr(), col.data_ptr(), val.data_ptr(), n_texts, kept_ptr.data_ptr(),
                                                         _opt(kept_class), _opt(kept_score), cap, res.data_ptr(), _opt_full(best), tmp.data_ptr(),
                                                         tmp.numel(), self._stream()), "acm_gpu_score_matrix_device")
                return Scored(kept_ptr, kept_class, kept_score, int(res.item()), best, kept_capacity=cap)
            return _counted(call, kept_capacity, "n_kept")

    def score_top(self, scored, n_classes, k):
        """acm_gpu_score_top_device(): TOP of a Scored of device tensors; returns it with class_hits, top_n, top_text and
        top_score ([n_classes, k]) filled in.  Queues only."""
        import torch
        n_classes, k = int(n_classes), int(k)
        kept_ptr = scored.kept_ptr
        assert kept_ptr.is_cuda and kept_ptr.is_contiguous() and kept_ptr.dtype == torch.int64
        dev = kept_ptr.device
        cap = int(scored.kept_class.numel()) if scored.kept_class is not None else 0
        hits, top_n, top_text, top_score = self._top_outputs(dev, n_classes, k)
        tmp = _scratch(lib().acm_gpu_score_top_tmp_bytes(self.h, cap, n_classes), dev)
        p = _opt_full
        _check(lib().acm_gpu_score_top_device(self.h, kept_ptr.data_ptr(), p(scored.kept_class), p(scored.kept_score), cap, kept_ptr.numel() - 1, n_classes,
                                              k, p(hits), p(top_n), p(top_text), p(top_score), tmp.data_ptr(), tmp.numel(), self._stream()),
               "acm_gpu_score_top_device")
        scored.class_hits, scored.top_n, scored.top_text, scored.top_score = hits, top_n, top_text, top_score
        scored._top_tmp = tmp                                                    # (the launches may still be queued)
        return scored

    def score_host(self, text, offsets, model, k=0):
        """acm_gpu_score_host(): the same as score() from host arrays, through the C ABI only (no torch).
        The call sizes its windows and its pair room itself.  Returns a Scored of numpy arrays."""
        t = np.ascontiguousarray(text)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        assert off.size >= 1, "offsets has n_texts + 1 entries"
        return _score_host_call(lib().acm_gpu_score_host, "acm_gpu_score_host", self.h, t, self.sym_size, off, model, k)

    def _index_keywords(self, n_keywords):
        return int(lib().acm_gpu_tally_keywords(self.h)) if n_keywords is None else int(n_keywords)

    def _post_outputs(self, dev, n_keywords, post_capacity):
        import torch
        post_text = torch.zeros(post_capacity, dtype=torch.int32, device=dev) if post_capacity else None
        return _i64(n_keywords + 1, dev), post_text, _i64(post_capacity, dev) if post_capacity else None

    def index(self, text, offsets, n_keywords=None, text_base=0, window=None, capacity=None, pair_capacity=None, post_capacity=None):
        """acm_gpu_index_device(): the inverted index of a batch on the device: the tally of tally_batch()
        (same `text`, `offsets`, `window`, `capacity`, `pair_capacity`) and the transposition behind it
        in one call; neither a record nor the count matrix leaves the device.  n_keywords (None: the
        plan's) may be larger; text ids start at text_base.  post_capacity: the room of post_text and
        post_count (0: count only, which gives post_ptr and so df; None: counted first, then sized by
        the count).  Returns an Indexed of device tensors; synchronises to read its four numbers."""
        n_symbols, n_texts = self._batch_args(text, offsets)
        window, capacity, pair_capacity = self._windows(window, capacity, pair_capacity)
        nk = self._index_keywords(n_keywords)
        dev = text.device
        res = _i64(6, dev)                                                       # nnz, total, need, need_pairs, forms[2]

        def call(cap):
            tmp = _scratch(lib().acm_gpu_index_tmp_bytes(self.h, window, capacity, pair_capacity, n_symbols, n_texts, nk, cap), dev)
            post_ptr, post_text, post_count = self._post_outputs(dev, nk, cap)
            _check(lib().acm_gpu_index_device(self.h, text.data_ptr(), n_symbols, offsets.data_ptr(), n_texts, window, capacity, pair_capacity, nk,
                                              int(text_base), post_ptr.data_ptr(), _opt(post_text), _opt(post_count), cap, res.data_ptr(),
                                              res.data_ptr() + 32, res.data_ptr() + 8, res.data_ptr() + 16, res.data_ptr() + 24, tmp.data_ptr(),
                                              tmp.numel(), self._stream()), "acm_gpu_index_device")
            nnz, total, need, need_pairs, fast, wide = (int(x) for x in res.cpu())
            return Indexed(post_ptr, post_text, post_count, nnz, total, int(text_base), need, need_pairs, cap, (fast, wide))
        return _counted(call, post_capacity, "nnz")

    def index_matrix(self, tallied, n_keywords=None, text_base=0, post_capacity=None):
        """acm_gpu_index_matrix_device(): the transposition of a count matrix that lies on the device:
        `tallied` is a TalliedBatch of device tensors, tally_batch()'s or the caller's own (row_ptr int64
        with n_texts + 1 entries, col int32, val int64).  Returns an Indexed of device tensors (total,
        need and need_pairs None); synchronises to read nnz."""
        row_ptr, col, val, n_texts = self._matrix_args(tallied)
        nk = self._index_keywords(n_keywords)
        dev = row_ptr.device
        res = _i64(3, dev)                                                       # nnz, forms[2]

        def call(cap):
            tmp = _scratch(lib().acm_gpu_index_matrix_tmp_bytes(self.h, n_texts, nk, cap), dev)
            post_ptr, post_text, post_count = self._post_outputs(dev, nk, cap)
            _check(lib().acm_gpu_index_matrix_device(self.h, row_ptr.data_ptr(), col.data_ptr(), val.data_ptr(), n_texts, nk, int(text_base),
                                                     post_ptr.data_ptr(), _opt(post_text), _opt(post_count), cap, res.data_ptr(), res.data_ptr() + 8,
                                                     tmp.data_ptr(), tmp.numel(), self._stream()), "acm_gpu_index_matrix_device")
            nnz, fast, wide = (int(x) for x in res.cpu())
            return Indexed(post_ptr, post_text, post_count, nnz, None, int(text_base), post_capacity=cap, forms=(fast, wide))
        return _counted(call, post_capacity, "nnz")

    def index_concat(self, a, b, out_capacity=None):
        """acm_gpu_index_concat_device(): per keyword a's list, then b's, for two Indexed of device
        tensors (a has no more keywords than b, and b's text ids lie above a's in every list).
        out_capacity None: a.nnz + b.nnz.  Returns an Indexed of device tensors; synchronises to read nnz."""
        import torch
        dev = a.post_ptr.device
        for x in (a, b):
            assert x.post_ptr.is_cuda and x.post_ptr.is_contiguous() and x.post_ptr.dtype == torch.int64
        nka, nkb = a.n_keywords, b.n_keywords
        cap = int(out_capacity) if out_capacity is not None else int(a.nnz) + int(b.nnz)
        res = _i64(1, dev)
        tmp = _scratch(lib().acm_gpu_index_concat_tmp_bytes(self.h, nkb), dev)
        out_ptr, out_text, out_count = self._post_outputs(dev, nkb, cap)
        p = _opt
        _check(lib().acm_gpu_index_concat_device(self.h, a.post_ptr.data_ptr(), p(a.post_text), p(a.post_count), nka, b.post_ptr.data_ptr(),
                                                 p(b.post_text), p(b.post_count), nkb, out_ptr.data_ptr(), p(out_text), p(out_count), cap,
                                                 res.data_ptr(), tmp.data_ptr(), tmp.numel(), self._stream()), "acm_gpu_index_concat_device")
        total = a.total + b.total if a.total is not None and b.total is not None else None
        return Indexed(out_ptr, out_text, out_count, int(res.item()), total, a.text_base, post_capacity=cap)

    def index_host(self, text, offsets, n_keywords=None, text_base=0):
        """acm_gpu_index_host(): the same as index() from host arrays, through the C ABI only (no torch).
        The call sizes its windows and its pair room itself.  Returns an Indexed of numpy arrays."""
        t = np.ascontiguousarray(text)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        assert off.size >= 1, "offsets has n_texts + 1 entries"
        return _index_host_call(lib().acm_gpu_index_host, "acm_gpu_index_host", self.h, t, self.sym_size, off, self._index_keywords(n_keywords), text_base)

    def _cooccur_outputs(self, dev, n_keywords, out_capacity):
        import torch
        co_col = torch.zeros(out_capacity, dtype=torch.int32, device=dev) if out_capacity else None
        return _i64(n_keywords + 1, dev), co_col, _i64(out_capacity, dev) if out_capacity else None

    @staticmethod
    def _cooccur_rooms(run, what, cross_capacity, out_capacity):
        """run(cross_capacity, out_capacity) -> a Cooccurred, for the device calls whose counts are read back: repeated
        with the cross room the device reported when that was too small and none was given, then -- out_capacity
        None -- counted first and sized by nnz"""
        room = [int(cross_capacity) if cross_capacity is not None else 1 << 16]

        def call(cap):
            got = run(room[0], cap)
            if got.cross > room[0] and cross_capacity is None:
                room[0] = got.cross
                got = run(room[0], cap)
            if got.cross > room[0]:
                e = ACMError(ACM_GPU_E_OVERFLOW, "%s: %d pair instances, room for %d" % (what, got.cross, room[0]))
                e.need = got.cross
                raise e
            return got
        return _counted(call, out_capacity, "nnz")

    def cooccur(self, text, offsets, flags=0, row_limit=0, n_keywords=None, window=None, capacity=None, pair_capacity=None, cross_capacity=None,
                out_capacity=None):
        """acm_gpu_cooccur_device(): the keyword co-occurrence matrix of a batch on the device: the tally of
        tally_batch() (same `text`, `offsets`, `window`, `capacity`, `pair_capacity`) and the pair passes
        behind it in one call, queued on the current stream; neither a record nor the count matrix leaves
        the device.  n_keywords (None: the plan's) may be larger.  cross_capacity: the room of the pair
        instances (None: 64 Ki, repeated once with what the device reports).  out_capacity: the room of
        co_col and co_val (0: count only, which gives co_ptr; None: counted first, then sized by the
        count).  Returns a Cooccurred of device tensors; synchronises to read its numbers.  Every repeat runs
        the whole call again, the tally included, with scratch of its own: with both rooms None that is up to
        three runs (the cross room reported, the count, the sized run).  A caller who knows the rooms of a
        batch, or takes them from the previous one (`cross`, `nnz`), passes both and pays for one."""
        n_symbols, n_texts = self._batch_args(text, offsets)
        window, capacity, pair_capacity = self._windows(window, capacity, pair_capacity)
        nk = self._index_keywords(n_keywords)
        flags = _cooccur_flags(flags)
        dev = text.device
        res = _i64(6, dev)                                                       # nnz, total, need, need_pairs, cross, skipped

        def run(cross_cap, cap):
            tmp = _scratch(lib().acm_gpu_cooccur_tmp_bytes(self.h, window, capacity, pair_capacity, n_symbols, n_texts, nk, cross_cap), dev)
            co_ptr, co_col, co_val = self._cooccur_outputs(dev, nk, cap)
            _check(lib().acm_gpu_cooccur_device(self.h, text.data_ptr(), n_symbols, offsets.data_ptr(), n_texts, window, capacity, pair_capacity, nk,
                                                flags, int(row_limit), cross_cap, co_ptr.data_ptr(), _opt(co_col), _opt(co_val), cap, res.data_ptr(),
                                                res.data_ptr() + 32, res.data_ptr() + 40, res.data_ptr() + 8, res.data_ptr() + 16,
                                                res.data_ptr() + 24, tmp.data_ptr(), tmp.numel(), self._stream()), "acm_gpu_cooccur_device")
            nnz, total, need, need_pairs, cross, skipped = (int(x) for x in res.cpu())
            return Cooccurred(co_ptr, co_col, co_val, nnz, cross, skipped, flags, total, int(row_limit), need, need_pairs, cap)
        return self._cooccur_rooms(run, "acm_gpu_cooccur_device", cross_capacity, out_capacity)

    def cooccur_matrix(self, tallied, flags=0, row_limit=0, n_keywords=None, cross_capacity=None, out_capacity=None):
        """acm_gpu_cooccur_matrix_device(): the co-occurrence matrix of a count matrix that lies on the
        device: `tallied` is a TalliedBatch of device tensors, tally_batch()'s or the caller's own (row_ptr
        int64 with n_texts + 1 entries, col int32 ascending within a row, val int64).  The rooms as in
        cooccur().  Returns a Cooccurred of device tensors (total, need and need_pairs None); synchronises
        to read its numbers."""
        row_ptr, col, val, n_texts = self._matrix_args(tallied)
        nk = self._index_keywords(n_keywords)
        flags = _cooccur_flags(flags)
        dev = row_ptr.device
        res = _i64(3, dev)                                                       # nnz, cross, skipped

        def run(cross_cap, cap):
            tmp = _scratch(lib().acm_gpu_cooccur_matrix_tmp_bytes(self.h, n_texts, nk, cross_cap), dev)
            co_ptr, co_col, co_val = self._cooccur_outputs(dev, nk, cap)
            _check(lib().acm_gpu_cooccur_matrix_device(self.h, row_ptr.data_ptr(), col.data_ptr(), val.data_ptr(), n_texts, nk, flags, int(row_limit),
                                                       cross_cap, co_ptr.data_ptr(), _opt(co_col), _opt(co_val), cap, res.data_ptr(),
                                                       res.data_ptr() + 8, res.data_ptr() + 16, tmp.data_ptr(), tmp.numel(), self._stream()),
                   "acm_gpu_cooccur_matrix_device")
            nnz, cross, skipped = (int(x) for x in res.cpu())
            return Cooccurred(co_ptr, co_col, co_val, nnz, cross, skipped, flags, None, int(row_limit), out_capacity=cap)
        return self._cooccur_rooms(run, "acm_gpu_cooccur_matrix_device", cross_capacity, out_capacity)

    def cooccur_add(self, a, b, cross_capacity=None, out_capacity=None):
        """acm_gpu_cooccur_add_device(): the entrywise sum of two Cooccurred of device tensors (a has no
        more keywords than b; both under the same flags and row_limit).  cross_capacity None: a.nnz +
        b.nnz, which always suffices; out_capacity None: the same, which cannot overflow.  Returns a
        Cooccurred of device tensors whose cross, skipped and total are the sums; synchronises to read nnz."""
        import torch
        dev = a.co_ptr.device
        for x in (a, b):
            assert x.co_ptr.is_cuda and x.co_ptr.is_contiguous() and x.co_ptr.dtype == torch.int64
        nka, nkb = a.n_keywords, b.n_keywords
        both = int(a.nnz) + int(b.nnz)
        cross_cap = int(cross_capacity) if cross_capacity is not None else both
        cap = int(out_capacity) if out_capacity is not None else both
        res = _i64(2, dev)                                                       # nnz, the cross room needed
        tmp = _scratch(lib().acm_gpu_cooccur_add_tmp_bytes(self.h, nkb, cross_cap), dev)
        out_ptr, out_col, out_val = self._cooccur_outputs(dev, nkb, cap)
        p = _opt
        _check(lib().acm_gpu_cooccur_add_device(self.h, a.co_ptr.data_ptr(), p(a.co_col), p(a.co_val), nka, b.co_ptr.data_ptr(), p(b.co_col),
                                                p(b.co_val), nkb, cross_cap, out_ptr.data_ptr(), p(out_col), p(out_val), cap, res.data_ptr(),
                                                res.data_ptr() + 8, tmp.data_ptr(), tmp.numel(), self._stream()), "acm_gpu_cooccur_add_device")
        nnz, need = (int(x) for x in res.cpu())
        if need > cross_cap:
            e = ACMError(ACM_GPU_E_OVERFLOW, "acm_gpu_cooccur_add_device: %d entries, room for %d" % (need, cross_cap))
            e.need = need
            raise e
        return Cooccurred(out_ptr, out_col, out_val, nnz, _sum_or_none(a.cross, b.cross), _sum_or_none(a.skipped, b.skipped), b.flags,
                          _sum_or_none(a.total, b.total), b.row_limit, out_capacity=cap)

    def cooccur_host(self, text, offsets, flags=0, row_limit=0, n_keywords=None):
        """acm_gpu_cooccur_host(): the same as cooccur() from host arrays, through the C ABI only (no torch).
        The call sizes its windows, its pair room and its cross room itself.  Returns a Cooccurred of numpy arrays."""
        t = np.ascontiguousarray(text)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        assert off.size >= 1, "offsets has n_texts + 1 entries"
        return _cooccur_host_call(lib().acm_gpu_cooccur_host, "acm_gpu_cooccur_host", self.h, t, self.sym_size, off, self._index_keywords(n_keywords),
                                  _cooccur_flags(flags), row_limit)

    def patterns_create(self, patternset):
        """acm_gpu_patterns_create(): `patternset` (a PatternSet, or lists of (keyword_id, offset, length)
        terms) compiled and uploaded to this plan's device.  Returns a Patterns; it stays valid across update()."""
        return Patterns.create(self, patternset)

    def patterns_records(self, records, n, patterns, n_symbols, offsets=None, pos_base=0, count=None, out=None, out_capacity=None, out_count=None):
        """acm_gpu_patterns_records_device(): the matches of `patterns` (a Patterns from patterns_create(), or a
        PatternSet compiled for this call) among records[:n] (an int64 [capacity, 2] device tensor in
        canonical order), into `out` (None: a new tensor of out_capacity records, by default n times the
        set's max_anchor_postings, which cannot overflow), queued on the current stream.  `count` (a device
        int64 tensor) gives the number of records on the device: n is the room of `records` then.
        `offsets` is a device int64 tensor of n_texts + 1 entries.  Returns (out, out_count): out_count (a
        device tensor) holds the number of matches; above out_capacity it is the capacity needed.  Nothing
        is synchronised."""
        return self._terms_records(Patterns, records, n, patterns, n_symbols, offsets, pos_base, count, out, out_capacity, out_count)

    def _terms_records(self, family, records, n, given, n_symbols, offsets, pos_base, count, out, out_capacity, out_count):
        """what patterns_records(), chains_records() and near_records() share, `family` being Patterns, Chains or Near: acm_gpu_<family>_tmp_bytes
        and acm_gpu_<family>_records_device"""
        import torch
        assert records.is_cuda and records.is_contiguous() and records.dtype == torch.int64 and records.shape[0] >= int(n)
        n = int(n)
        call = "acm_gpu_%s_records_device" % family.STEM
        with family.for_call(self, given, sync=True) as S:
            if out_capacity is None:
                out_capacity = out.shape[0] if out is not None else n * S.info()[family.MOST]
            out_capacity = int(out_capacity)
            if out is None:
                out = torch.empty((max(out_capacity, 1), 2), dtype=torch.int64, device=records.device)
            assert out.is_cuda and out.is_contiguous() and out.shape[0] >= out_capacity
            if out_count is None:
                out_count = _i64(1, records.device)
            off_ptr, n_texts = _cut(offsets)
            tmp = _scratch(getattr(lib(), "acm_gpu_%s_tmp_bytes" % family.STEM)(self.h, S.h, n, n_texts), records.device)
            _check(getattr(lib(), call)(self.h, S.h, records.data_ptr(), n, _opt(count), int(n_symbols), int(pos_base), off_ptr, n_texts,
                                        out.data_ptr() if out_capacity else None, out_capacity, out_count.data_ptr(), tmp.data_ptr(), tmp.numel(),
                                        self._stream()), call)
            return out, out_count

    def scan_patterns(self, text, patterns, offsets=None, n_symbols=None, pos_base=0, capacity=None, out=None, out_capacity=None, tmp=None):
        """acm_gpu_scan_patterns_device(): the ordered scan of a device tensor into `capacity` records of the
        call's own and the matches of `patterns` among them, queued on the current stream.  Returns (out,
        count, found, tmp) with count and found device tensors: out[:count] are the matches when count <=
        out_capacity; found is the scan's count -- above `capacity` there is no match (count 0) and found
        is a capacity that suffices."""
        return self._scan_terms(Patterns, text, patterns, offsets, n_symbols, pos_base, capacity, out, out_capacity, tmp)

    def _scan_terms(self, family, text, given, offsets, n_symbols, pos_base, capacity, out, out_capacity, tmp):
        """what scan_patterns(), scan_chains() and scan_near() share, `family` being Patterns, Chains or Near: acm_gpu_scan_<family>_tmp_bytes
        and acm_gpu_scan_<family>_device"""
        import torch
        n_symbols = self._text_args(text, n_symbols)
        call = "acm_gpu_scan_%s_device" % family.STEM
        capacity = int(capacity) if capacity is not None else max(4096, n_symbols // 256)
        with family.for_call(self, given, sync=True) as S:
            if out_capacity is None:
                out_capacity = out.shape[0] if out is not None else capacity * S.info()[family.MOST]
            out_capacity = int(out_capacity)
            if out is None:
                out = torch.empty((max(out_capacity, 1), 2), dtype=torch.int64, device=text.device)
            res = _i64(2, text.device)
            off_ptr, n_texts = _cut(offsets)
            tmp = _scratch(getattr(lib(), "acm_gpu_scan_%s_tmp_bytes" % family.STEM)(self.h, S.h, capacity, n_symbols, n_texts), text.device, tmp)
            _check(getattr(lib(), call)(self.h, S.h, text.data_ptr(), n_symbols, int(pos_base), off_ptr, n_texts, capacity,
                                        out.data_ptr() if out_capacity else None, out_capacity, res.data_ptr(), res.data_ptr() + 8,
                                        tmp.data_ptr(), tmp.numel(), self._stream()), call)
            return out, res[0:1], res[1:2], tmp

    def scan_patterns_host(self, text, patternset, offsets=None, pos_base=0, out_capacity=None):
        """acm_gpu_scan_patterns_host(): numpy in, the pattern matches out, through the C ABI only (no torch); an
        overflow is repeated once with the size the call reports."""
        return self._scan_set_host("acm_gpu_scan_patterns_host", text, _patternset(patternset), offsets, pos_base, out_capacity, extra=())[0]

    def chains_create(self, chainset):
        """acm_gpu_chains_create(): `chainset` (a ChainSet, or lists of (keyword_id, gap_min, gap_max) terms)
        compiled and uploaded to this plan's device.  Returns a Chains; it stays valid across update()."""
        return Chains.create(self, chainset)

    def chains_records(self, records, n, chains, n_symbols, offsets=None, pos_base=0, count=None, out=None, out_capacity=None, out_count=None):
        """acm_gpu_chains_records_device(): the matches of `chains` (a Chains from chains_create(), or a
        ChainSet compiled for this call) among records[:n] (an int64 [capacity, 2] device tensor in
        canonical order), into `out` (None: a new tensor of out_capacity records, by default n times the
        set's max_last_postings, which cannot overflow), queued on the current stream.  `count` (a device
        int64 tensor) gives the number of records on the device: n is the room of `records` then.
        `offsets` is a device int64 tensor of n_texts + 1 entries.  Returns (out, out_count): out_count (a
        device tensor) holds the number of matches; above out_capacity it is the capacity needed.  Nothing
        is synchronised."""
        return self._terms_records(Chains, records, n, chains, n_symbols, offsets, pos_base, count, out, out_capacity, out_count)

    def scan_chains(self, text, chains, offsets=None, n_symbols=None, pos_base=0, capacity=None, out=None, out_capacity=None, tmp=None):
        """acm_gpu_scan_chains_device(): the ordered scan of a device tensor into `capacity` records of the
        call's own and the matches of `chains` among them, queued on the current stream.  Returns (out,
        count, found, tmp) with count and found device tensors: out[:count] are the matches when count <=
        out_capacity; found is the scan's count -- above `capacity` there is no match (count 0) and found
        is a capacity that suffices."""
        return self._scan_terms(Chains, text, chains, offsets, n_symbols, pos_base, capacity, out, out_capacity, tmp)

    def scan_chains_host(self, text, chainset, offsets=None, pos_base=0, out_capacity=None):
        """acm_gpu_scan_chains_host(): numpy in, the chain matches out, through the C ABI only (no torch); an
        overflow is repeated once with the size the call reports."""
        return self._scan_set_host("acm_gpu_scan_chains_host", text, _chainset(chainset), offsets, pos_base, out_capacity, extra=())[0]

    def near(self, nearset):
        """acm_gpu_near_create(): `nearset` (a NearSet, or what makes one) compiled and uploaded to this plan's
        device.  Returns a Near; it stays valid across update()."""
        return Near.create(self, nearset)

    def near_records(self, records, n, near, n_symbols, offsets=None, pos_base=0, count=None, out=None, out_capacity=None, out_count=None):
        """acm_gpu_near_records_device(): the matches of `near` (a Near from near(), or a NearSet compiled for
        this call) among records[:n]; arguments and results as chains_records(), the default out_capacity
        being n times the set's max_postings, which cannot overflow.  Nothing is synchronised."""
        return self._terms_records(Near, records, n, near, n_symbols, offsets, pos_base, count, out, out_capacity, out_count)

    def scan_near(self, text, near, offsets=None, n_symbols=None, pos_base=0, capacity=None, out=None, out_capacity=None, tmp=None):
        """acm_gpu_scan_near_device(): the ordered scan of a device tensor into `capacity` records of the call's
        own and the matches of `near` among them, queued on the current stream; arguments and results as
        scan_chains()."""
        return self._scan_terms(Near, text, near, offsets, n_symbols, pos_base, capacity, out, out_capacity, tmp)

    def scan_near_host(self, text, nearset, offsets=None, pos_base=0, out_capacity=None):
        """acm_gpu_scan_near_host(): numpy in, the NEAR matches out, through the C ABI only (no torch); an
        overflow is repeated once with the size the call reports."""
        return self._scan_set_host("acm_gpu_scan_near_host", text, _nearset(nearset), offsets, pos_base, out_capacity, extra=())[0]

    def approx_create(self, approxset):
        """acm_gpu_approx_create(): `approxset` (an ApproxSet) compiled and uploaded to this plan's device.
        Returns an Approx; it stays valid across update().  A plan over comparator classes refuses
        (ACM_GPU_E_INELIGIBLE)."""
        return Approx.create(self, approxset)

    def templates_create(self, templateset):
        """acm_gpu_templates_create(): `templateset` (a TemplateSet) compiled and uploaded to this plan's device.
        Returns a Templates; it stays valid across update().  A plan over comparator classes refuses
        (ACM_GPU_E_INELIGIBLE)."""
        return Templates.create(self, templateset)

    def _approx_for_call(self, approx):
        """the Approx or Templates of one call: `approx` itself, or an ApproxSet or a TemplateSet compiled for it (an
        Approx is what the calls take; a Templates is one)"""
        return (Templates if isinstance(approx, TemplateSet) else Approx).for_call(self, approx, sync=True)

    def templates_records(self, records, n, templates, text, n_symbols=None, offsets=None, pos_base=0, count=None, out=None, dist=None,
                          out_capacity=None, out_count=None):
        """acm_gpu_templates_records_device(): the matches of the templates of `templates` (a Templates from
        templates_create(), or a TemplateSet compiled for this call) that records[:n] seed; arguments and return as
        approx_records()."""
        return self._set_records("templates", records, n, templates, text, n_symbols, offsets, pos_base, count, out, dist, out_capacity, out_count)

    def scan_templates(self, text, templates, offsets=None, n_symbols=None, pos_base=0, capacity=None, out=None, dist=None, out_capacity=None, tmp=None):
        """acm_gpu_scan_templates_device(): the ordered scan of a device tensor and the templates of `templates` verified
        around its records; arguments and return as scan_approx()."""
        return self._scan_set("templates", text, templates, offsets, n_symbols, pos_base, capacity, out, dist, out_capacity, tmp)

    def scan_templates_host(self, text, templateset, offsets=None, pos_base=0, out_capacity=None):
        """acm_gpu_scan_templates_host(): numpy in, (matches, dist) out; arguments as scan_approx_host()."""
        return self._scan_set_host("acm_gpu_scan_templates_host", text, templateset, offsets, pos_base, out_capacity)

    def approx_records(self, records, n, approx, text, n_symbols=None, offsets=None, pos_base=0, count=None, out=None, dist=None, out_capacity=None,
                       out_count=None):
        """acm_gpu_approx_records_device(): the occurrences with at most k mismatches of the targets of `approx`
        (an Approx from approx_create(), or an ApproxSet compiled for this call) that records[:n] seed (an int64
        [capacity, 2] device tensor in canonical order) in `text` (a device tensor of the caller's symbols), into
        `out` and `dist` (None: new tensors of out_capacity entries, by default n times the set's max_postings,
        which cannot overflow), queued on the current stream.  `count` (a device int64 tensor) gives the number of
        records on the device: n is the room of `records` then.  `offsets` is a device int64 tensor of n_texts + 1
        entries.  Returns (out, dist, out_count): out_count (a device tensor) holds the number of matches; above
        out_capacity it is the capacity needed.  Nothing is synchronised."""
        return self._set_records("approx", records, n, approx, text, n_symbols, offsets, pos_base, count, out, dist, out_capacity, out_count)

    def edit_records(self, records, n, approx, text, n_symbols=None, offsets=None, pos_base=0, count=None, out=None, dist=None, out_capacity=None,
                     out_count=None):
        """acm_gpu_edit_records_device(): the ends at which the targets of `approx` occur within edit distance k among
        those records[:n] seed; arguments and return as approx_records().  out_capacity defaults to n times the
        set's max_postings times 2 max_k + 1, which cannot overflow.  A set with a budget above 15, or not below
        its target's length, is refused (ACM_GPU_E_ARG)."""
        return self._set_records("edit", records, n, approx, text, n_symbols, offsets, pos_base, count, out, dist, out_capacity, out_count)

    @staticmethod
    def _most_per_record(metric, info):
        """the matches one record can seed, from acm_gpu_approx_info()'s figures"""
        return info["max_postings"] * (2 * info["max_k"] + 1 if metric == "edit" else 1)

    def _set_records(self, metric, records, n, approx, text, n_symbols, offsets, pos_base, count, out, dist, out_capacity, out_count):
        """what approx_records() and edit_records() share: acm_gpu_<metric>_tmp_bytes and acm_gpu_<metric>_records_device"""
        import torch
        assert records.is_cuda and records.is_contiguous() and records.dtype == torch.int64 and records.shape[0] >= int(n)
        n = int(n)
        call = "acm_gpu_%s_records_device" % metric
        n_symbols = self._text_args(text, n_symbols)
        with self._approx_for_call(approx) as A:
            if out_capacity is None:
                out_capacity = out.shape[0] if out is not None else n * self._most_per_record(metric, A.info())
            out_capacity = int(out_capacity)
            if out is None:
                out = torch.empty((max(out_capacity, 1), 2), dtype=torch.int64, device=records.device)
            if dist is None:
                dist = torch.empty(max(out_capacity, 1), dtype=torch.int32, device=records.device)
            assert out.is_cuda and out.is_contiguous() and out.shape[0] >= out_capacity and dist.is_cuda and dist.numel() >= out_capacity
            if out_count is None:
                out_count = _i64(1, records.device)
            off_ptr, n_texts = _cut(offsets)
            tmp = _scratch(getattr(lib(), "acm_gpu_%s_tmp_bytes" % metric)(self.h, A.h, n, out_capacity, n_texts), records.device)
            _check(getattr(lib(), call)(self.h, A.h, records.data_ptr(), n, _opt(count), text.data_ptr(), int(n_symbols), int(pos_base), off_ptr,
                                        n_texts, out.data_ptr() if out_capacity else None, dist.data_ptr(), out_capacity,
                                        out_count.data_ptr(), tmp.data_ptr(), tmp.numel(), self._stream()), call)
            return out, dist, out_count

    def scan_approx(self, text, approx, offsets=None, n_symbols=None, pos_base=0, capacity=None, out=None, dist=None, out_capacity=None, tmp=None):
        """acm_gpu_scan_approx_device(): the ordered scan of a device tensor into `capacity` records of the call's
        own and the targets of `approx` verified around them, queued on the current stream.  Returns (out, dist,
        count, found, tmp) with count and found device tensors: out[:count] and dist[:count] are the matches when
        count <= out_capacity; found is the scan's count -- above `capacity` there is no match (count 0) and found
        is a capacity that suffices."""
        return self._scan_set("approx", text, approx, offsets, n_symbols, pos_base, capacity, out, dist, out_capacity, tmp)

    def scan_edit(self, text, approx, offsets=None, n_symbols=None, pos_base=0, capacity=None, out=None, dist=None, out_capacity=None, tmp=None):
        """acm_gpu_scan_edit_device(): the ordered scan of a device tensor and the targets of `approx` verified within
        edit distance k around its records; arguments and return as scan_approx()."""
        return self._scan_set("edit", text, approx, offsets, n_symbols, pos_base, capacity, out, dist, out_capacity, tmp)

    def _scan_set(self, metric, text, approx, offsets, n_symbols, pos_base, capacity, out, dist, out_capacity, tmp):
        """what scan_approx() and scan_edit() share: acm_gpu_scan_<metric>_tmp_bytes and acm_gpu_scan_<metric>_device"""
        import torch
        call = "acm_gpu_scan_%s_device" % metric
        n_symbols = self._text_args(text, n_symbols)
        capacity = int(capacity) if capacity is not None else max(4096, n_symbols // 256)
        with self._approx_for_call(approx) as A:
            if out_capacity is None:
                out_capacity = out.shape[0] if out is not None else capacity * self._most_per_record(metric, A.info())
            out_capacity = int(out_capacity)
            if out is None:
                out = torch.empty((max(out_capacity, 1), 2), dtype=torch.int64, device=text.device)
            if dist is None:
                dist = torch.empty(max(out_capacity, 1), dtype=torch.int32, device=text.device)
            res = _i64(2, text.device)
            off_ptr, n_texts = _cut(offsets)
            tmp = _scratch(getattr(lib(), "acm_gpu_scan_%s_tmp_bytes" % metric)(self.h, A.h, capacity, out_capacity, n_symbols, n_texts), text.device, tmp)
            _check(getattr(lib(), call)(self.h, A.h, text.data_ptr(), n_symbols, int(pos_base), off_ptr, n_texts, capacity,
                                        out.data_ptr() if out_capacity else None, dist.data_ptr(), out_capacity, res.data_ptr(),
                                        res.data_ptr() + 8, tmp.data_ptr(), tmp.numel(), self._stream()), call)
            return out, dist, res[0:1], res[1:2], tmp

    def scan_approx_host(self, text, approxset, offsets=None, pos_base=0, out_capacity=None):
        """acm_gpu_scan_approx_host(): numpy in, (matches, dist) out, through the C ABI only (no torch); an overflow
        is repeated once with the size the call reports."""
        return self._scan_set_host("acm_gpu_scan_approx_host", text, approxset, offsets, pos_base, out_capacity)

    def scan_edit_host(self, text, approxset, offsets=None, pos_base=0, out_capacity=None):
        """acm_gpu_scan_edit_host(): numpy in, (matches, dist) within edit distance k out; arguments as scan_approx_host()."""
        return self._scan_set_host("acm_gpu_scan_edit_host", text, approxset, offsets, pos_base, out_capacity)

    def _scan_set_host(self, name, text, tset, offsets, pos_base, out_capacity, extra=(np.uint32,)):
        """what the host scans for the sets of a family share -- patterns and chains, and with a distance per match
        (`extra`) approx, edit and templates --: the blocking C call `name`"""
        t = np.ascontiguousarray(text)
        n_sym = t.size * t.itemsize // self.sym_size
        off = np.ascontiguousarray(offsets, dtype=np.uint64) if offsets is not None else None
        return _matches_host_call(getattr(lib(), name), name, (self.h, _ptr(t), n_sym, int(pos_base), *_cut(off), *tset.args()), out_capacity, extra)

    @property
    def select_form(self):
        """acm_gpu_select_form(): 1 = the plan's selections go by tiles of candidates in LDS, 2 = by the
        walk through global memory (a keyword longer than a tile, or ACM_GPU_SELECT=walk)."""
        return int(lib().acm_gpu_select_form(self.h))

    def select_records(self, records, n, pos_lo, span, out=None):
        """acm_gpu_select_records_device(): SELECT of the first n records of `records` (an int64
        [capacity, 2] device tensor in canonical order, every start and end in [pos_lo, pos_lo +
        span)) into `out` (None: a new tensor; may be `records` itself).  Returns (out, count): the
        selected records are out[:count].  Synchronises to read the count."""
        import torch
        assert records.is_cuda and records.is_contiguous() and records.dtype == torch.int64
        n = int(n)
        if out is None:
            out = torch.empty((max(n, 1), 2), dtype=torch.int64, device=records.device)
        assert out.is_cuda and out.is_contiguous() and out.shape[0] >= n and records.shape[0] >= n
        count = _i64(1, records.device)
        tmp = _scratch(lib().acm_gpu_select_tmp_bytes(self.h, n, span), records.device)
        _check(lib().acm_gpu_select_records_device(self.h, records.data_ptr(), n, None, pos_lo, span, out.data_ptr(), count.data_ptr(),
                                                   tmp.data_ptr(), tmp.numel(), self._stream()), "acm_gpu_select_records_device")
        return out, int(count.item())

    def scan_select(self, text, n_symbols=None, pos_base=0, capacity=None, records=None, count=None, tmp=None):
        """acm_gpu_scan_select_device(): the ordered scan of a device tensor and the leftmost-longest
        selection of its records, queued on the current stream.  Returns (records, count, tmp):
        records[:count] is the selection when count <= capacity; a greater count is the number of ALL
        matches, the capacity the call needs."""
        n_symbols = self._text_args(text, n_symbols)
        records, count = self._records_out(records, count, capacity, n_symbols, text.device)
        tmp = _scratch(lib().acm_gpu_scan_select_tmp_bytes(self.h, records.shape[0], n_symbols), text.device, tmp)
        _check(lib().acm_gpu_scan_select_device(self.h, text.data_ptr(), n_symbols, pos_base, records.data_ptr(), records.shape[0],
                                                count.data_ptr(), tmp.data_ptr(), tmp.numel(), self._stream()),
               "acm_gpu_scan_select_device")
        return records, count, tmp

    def segment_records(self, records, n, pos_lo, span, cost, gap_cost, out=None, count=None, sums=None):
        """acm_gpu_segment_records_device(): SEGMENT of records[:n] (an int64 [capacity, 2] device tensor
        in canonical order, every start and end in [pos_lo, pos_lo + span)) under `cost` (a device
        tensor of int32 / uint32 words, one per keyword) and gap_cost, into `out` (None: a new tensor;
        may be `records` itself).  `count` (a device tensor of one int64, None: n is the count) holds
        the number of records on the way in and of selected records on the way out.  Returns (out,
        count, sums): Python ints read after a synchronise, sums = (cost, lengths)."""
        import torch
        assert records.is_cuda and records.is_contiguous() and records.dtype == torch.int64
        assert cost.is_cuda and cost.is_contiguous() and cost.element_size() == 4
        room = int(records.shape[0]) if count is not None else int(n)
        if out is None:
            out = torch.empty((max(room, 1), 2), dtype=torch.int64, device=records.device)
        assert out.is_cuda and out.is_contiguous() and out.shape[0] >= room and records.shape[0] >= room
        d_count = count if count is not None else _i64(1, records.device)
        if sums is None:
            sums = _i64(2, records.device)
        tmp = _scratch(lib().acm_gpu_segment_tmp_bytes(self.h, room, span), records.device)
        _check(lib().acm_gpu_segment_records_device(self.h, records.data_ptr(), room, _opt(count), pos_lo, span,
                                                    cost.data_ptr(), cost.numel(), int(gap_cost), out.data_ptr(), d_count.data_ptr(),
                                                    sums.data_ptr(), tmp.data_ptr(), tmp.numel(), self._stream()),
               "acm_gpu_segment_records_device")
        return out, int(d_count.item()), (int(sums[0].item()), int(sums[1].item()))

    def scan_segment(self, text, cost, gap_cost, offsets=None, n_symbols=None, pos_base=0, capacity=None, records=None, count=None, sums=None,
                     tmp=None):
        """acm_gpu_scan_segment_device(): the ordered scan of a device tensor (offsets, a device tensor of
        int64 [n_texts + 1]: the batch scan) and the minimum-cost tiling of its records, queued on the
        current stream.  Returns (records, count, sums, tmp): records[:count] is the tiling when count
        <= capacity; a greater count is the number of ALL matches, the capacity the call needs."""
        import torch
        assert text.is_cuda and text.is_contiguous() and cost.is_cuda and cost.is_contiguous() and cost.element_size() == 4
        n_symbols = self._text_args(text, n_symbols)
        records, count = self._records_out(records, count, capacity, n_symbols, text.device)
        if sums is None:
            sums = _i64(2, text.device)
        assert offsets is None or (offsets.is_cuda and offsets.is_contiguous() and offsets.dtype == torch.int64)
        off_ptr, n_texts = _cut(offsets)
        tmp = _scratch(lib().acm_gpu_scan_segment_tmp_bytes(self.h, records.shape[0], n_symbols, n_texts), text.device, tmp)
        _check(lib().acm_gpu_scan_segment_device(self.h, text.data_ptr(), n_symbols, pos_base, off_ptr,
                                                 n_texts, cost.data_ptr(), cost.numel(), int(gap_cost), records.data_ptr(), records.shape[0],
                                                 count.data_ptr(), sums.data_ptr(), tmp.data_ptr(), tmp.numel(), self._stream()),
               "acm_gpu_scan_segment_device")
        return records, count, sums, tmp

    def scan_segment_host(self, text, cost, gap_cost, offsets=None, pos_base=0, capacity=None):
        """acm_gpu_scan_segment_host(): numpy in, (records, sums) out, through the C ABI only (no torch);
        an overflow is repeated once with the size the call reports."""
        t = np.ascontiguousarray(text)
        n_sym = t.size * t.itemsize // self.sym_size
        off = np.ascontiguousarray(offsets, dtype=np.uint64) if offsets is not None else None
        return _segment_host_call(lib().acm_gpu_scan_segment_host, "acm_gpu_scan_segment_host", (self.h, t.ctypes.data, n_sym, pos_base, *_cut(off)),
                                  cost, gap_cost, int(capacity) if capacity is not None else max(1024, n_sym // 64), capacity is not None)

    def scan_select_host(self, text, pos_base=0, capacity=None):
        """acm_gpu_scan_select_host(): numpy in, the selected records out, through the C ABI only (no
        torch); an overflow is repeated once with the size the call reports."""
        t = np.ascontiguousarray(text)
        n_sym = t.size * t.itemsize // self.sym_size
        return _records_host_call(lib().acm_gpu_scan_select_host, "acm_gpu_scan_select_host", (self.h, t.ctypes.data, n_sym, pos_base),
                                  int(capacity) if capacity is not None else max(1024, n_sym // 64), capacity is not None)

    def words_records(self, text, records, n, offsets=None, ranges=ASCII_WORD, flags="both", pos_base=0, n_symbols=None, out=None, count=None,
                      out_count=None):
        """acm_gpu_words_records_device(): the whole-word records (see words_records) of records[:n] (an
        int64 [capacity, 2] device tensor, any order) over `text` (a device tensor), into `out` (None:
        a new tensor; it must not overlap `records`), queued on the current stream.  `count` (a device
        int64 tensor) gives the number of records on the device: n is the room of `records` and `out`
        then.  `offsets` is a device int64 tensor of n_texts + 1 entries.  Returns (out, out_count):
        out_count (None: a new device tensor; may be `count`) holds the number of kept records, or
        `count`'s value when that exceeds n.  Nothing is synchronised."""
        import torch
        n_symbols = self._text_args(text, n_symbols)
        assert records.is_cuda and records.is_contiguous() and records.dtype == torch.int64 and records.shape[0] >= int(n)
        n = int(n)
        if out is None:
            out = torch.empty((max(n, 1), 2), dtype=torch.int64, device=records.device)
        assert out.is_cuda and out.is_contiguous() and out.shape[0] >= n
        if out_count is None:
            out_count = _i64(1, records.device)
        r, nr = _word_ranges(ranges, self.sym_size)
        off_ptr, n_texts = _cut(offsets)
        tmp = _scratch(lib().acm_gpu_words_tmp_bytes(self.h, n, n_texts), records.device)
        _check(lib().acm_gpu_words_records_device(self.h, text.data_ptr(), n_symbols, pos_base, off_ptr, n_texts, r.ctypes.data, nr, _word_flags(flags),
                                                  records.data_ptr(), n, _opt(count), out.data_ptr(), out_count.data_ptr(), tmp.data_ptr(),
                                                  tmp.numel(), self._stream()), "acm_gpu_words_records_device")
        return out, out_count

    def scan_words(self, text, offsets=None, ranges=ASCII_WORD, flags="both", n_symbols=None, pos_base=0, capacity=None, records=None, count=None,
                   tmp=None):
        """acm_gpu_scan_words_device(): the ordered scan of a device tensor and the whole-word filter of
        its records, queued on the current stream.  Returns (records, count, tmp): records[:count] are
        the whole-word matches in canonical order when count <= capacity; a greater count is the
        number of ALL matches, the capacity the call needs."""
        n_symbols = self._text_args(text, n_symbols)
        records, count = self._records_out(records, count, capacity, n_symbols, text.device)
        r, nr = _word_ranges(ranges, self.sym_size)
        off_ptr, n_texts = _cut(offsets)
        tmp = _scratch(lib().acm_gpu_scan_words_tmp_bytes(self.h, records.shape[0], n_symbols, n_texts), text.device, tmp)
        _check(lib().acm_gpu_scan_words_device(self.h, text.data_ptr(), n_symbols, pos_base, off_ptr,
                                               n_texts, r.ctypes.data, nr, _word_flags(flags), records.data_ptr(), records.shape[0],
                                               count.data_ptr(), tmp.data_ptr(), tmp.numel(), self._stream()), "acm_gpu_scan_words_device")
        return records, count, tmp

    def scan_words_host(self, text, offsets=None, ranges=ASCII_WORD, flags="both", pos_base=0, capacity=None):
        """acm_gpu_scan_words_host(): numpy in, the whole-word records out, through the C ABI only (no
        torch); an overflow is repeated once with the size the call reports."""
        t = np.ascontiguousarray(text)
        n_sym = t.size * t.itemsize // self.sym_size
        r, nr = _word_ranges(ranges, self.sym_size)
        off = np.ascontiguousarray(offsets, dtype=np.uint64) if offsets is not None else None
        return _records_host_call(lib().acm_gpu_scan_words_host, "acm_gpu_scan_words_host",
                                  (self.h, _ptr(t), n_sym, pos_base, *_cut(off), r.ctypes.data, nr, _word_flags(flags)),
                                  int(capacity) if capacity is not None else max(1024, n_sym // 64), capacity is not None)

    def chars_ruler(self, text, n_symbols=None, ruler=None, tmp=None):
        """acm_gpu_chars_ruler_device(): the rank structure of the UTF-8 bytes `text` (a device tensor) that
        chars_records and chars_positions read, queued on the current stream.  It belongs to `text` as it lies: hand
        the same tensor to those calls.  Returns the ruler (a uint8 device tensor; `ruler`: an earlier one to build in)."""
        import torch
        n_symbols = self._text_args(text, n_symbols)
        rb = lib().acm_gpu_chars_ruler_bytes(self.h, n_symbols)
        if not rb:
            raise ACMError(ACM_GPU_E_ARG, "acm_gpu_chars_ruler_bytes")
        if ruler is None or ruler.numel() < rb:
            ruler = torch.empty(rb, dtype=torch.uint8, device=text.device)
        tmp = _scratch(lib().acm_gpu_chars_ruler_tmp_bytes(self.h, n_symbols), text.device, tmp)
        _check(lib().acm_gpu_chars_ruler_device(self.h, _opt_full(text), n_symbols, ruler.data_ptr(), ruler.numel(), tmp.data_ptr(), tmp.numel(),
                                                self._stream()), "acm_gpu_chars_ruler_device")
        return ruler

    def chars_records(self, text, ruler, records, n, offsets=None, unit="codepoints", pos_base=0, n_symbols=None, count=None, char_start=None,
                      char_len=None, edge=None):
        """acm_gpu_chars_records_device(): where records[:n] (an int64 [capacity, 2] device tensor, any order) over
        `text` lie in code points or UTF-16 code units (see chars_records), by `ruler` (chars_ruler(text)), queued on the
        current stream.  `count` (a device int64 tensor) gives the number of records on the device: n is the room
        then.  Returns (char_start int64, char_len int32, edge uint8) device tensors, one entry per record.  Nothing is
        synchronised."""
        import torch
        n_symbols = self._text_args(text, n_symbols)
        assert records.is_cuda and records.is_contiguous() and records.dtype == torch.int64 and records.shape[0] >= int(n)
        n, dev = int(n), records.device
        char_start = char_start if char_start is not None else torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        char_len = char_len if char_len is not None else torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        edge = edge if edge is not None else torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        off_ptr, n_texts = _cut(offsets)
        tmp = _scratch(lib().acm_gpu_chars_tmp_bytes(self.h, n, n_texts), dev)
        _check(lib().acm_gpu_chars_records_device(self.h, _opt_full(text), n_symbols, pos_base, off_ptr, n_texts, _chars_unit(unit), ruler.data_ptr(),
                                                  records.data_ptr(), n, _opt(count), char_start.data_ptr(), char_len.data_ptr(), edge.data_ptr(),
                                                  tmp.data_ptr(), tmp.numel(), self._stream()), "acm_gpu_chars_records_device")
        return char_start, char_len, edge

    def chars_positions(self, text, ruler, positions, offsets=None, unit="codepoints", n_symbols=None, out=None):
        """acm_gpu_chars_positions_device(): the byte positions `positions` (a device int64 tensor, 0 .. n_symbols) in
        code points or UTF-16 code units from the beginning of their text, by `ruler`, queued on the current stream:
        the way the outputs of the other families (a selection's records, token places, snippet bounds) reach the
        caller's units through one ruler.  Returns `out`, a device int64 tensor."""
        import torch
        n_symbols = self._text_args(text, n_symbols)
        assert positions.is_cuda and positions.is_contiguous() and positions.dtype == torch.int64
        n = positions.numel()
        if out is None:
            out = torch.empty(max(n, 1), dtype=torch.int64, device=positions.device)
        off_ptr, n_texts = _cut(offsets)
        tmp = _scratch(lib().acm_gpu_chars_tmp_bytes(self.h, n, n_texts), positions.device)
        _check(lib().acm_gpu_chars_positions_device(self.h, _opt_full(text), n_symbols, off_ptr, n_texts, _chars_unit(unit), ruler.data_ptr(),
                                                    _opt_full(positions), n, out.data_ptr(), tmp.data_ptr(), tmp.numel(), self._stream()),
               "acm_gpu_chars_positions_device")
        return out

    def scan_chars(self, text, offsets=None, unit="codepoints", n_symbols=None, pos_base=0, capacity=None, records=None, count=None, tmp=None):
        """acm_gpu_scan_chars_device(): the ordered scan of a device tensor of UTF-8 bytes, its ruler and the map of
        its records, queued on the current stream.  Returns (records, char_start, char_len, edge, count, tmp):
        their first `count` entries count when count <= capacity; a greater count is the number of ALL matches, the
        capacity the call needs."""
        import torch
        n_symbols = self._text_args(text, n_symbols)
        records, count = self._records_out(records, count, capacity, n_symbols, text.device)
        cap, dev = records.shape[0], text.device
        char_start = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        char_len = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        edge = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        off_ptr, n_texts = _cut(offsets)
        tmp = _scratch(lib().acm_gpu_scan_chars_tmp_bytes(self.h, cap, n_symbols, n_texts), dev, tmp)
        _check(lib().acm_gpu_scan_chars_device(self.h, _opt_full(text), n_symbols, pos_base, off_ptr, n_texts, _chars_unit(unit), records.data_ptr(),
                                               char_start.data_ptr(), char_len.data_ptr(), edge.data_ptr(), cap, count.data_ptr(), tmp.data_ptr(),
                                               tmp.numel(), self._stream()), "acm_gpu_scan_chars_device")
        return records, char_start, char_len, edge, count, tmp

    def scan_chars_host(self, text, offsets=None, unit="codepoints", pos_base=0, capacity=None):
        """acm_gpu_scan_chars_host(): numpy in, (records, char_start, char_len, edge) out, through the C ABI only (no
        torch); an overflow is repeated once with the size the call reports."""
        t = np.frombuffer(bytes(text), np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text)
        n_sym = t.size * t.itemsize // self.sym_size
        off = np.ascontiguousarray(offsets, dtype=np.uint64) if offsets is not None else None
        return _chars_host_call(lib().acm_gpu_scan_chars_host, "acm_gpu_scan_chars_host", (self.h, _ptr(t), n_sym, pos_base, *_cut(off), _chars_unit(unit)),
                                int(capacity) if capacity is not None else max(1024, n_sym // 64), capacity is not None)

    def _context_outputs(self, text, room, n_symbols, gather, out, out_capacity):
        """the device outputs of the context calls: (snip_lo, out_offsets, snip_text, rec_snip, rec_at, res, out, out_capacity);
        res = the record count, n_snippets, out_symbols"""
        import torch
        dev = text.device
        i64 = lambda n: torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
        i32 = lambda n: torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        return (i64(room), i64(room + 1), i32(room), i32(room), i64(room), i64(3), *self._gather_room(dev, gather, out, out_capacity, n_symbols))

    def context_records(self, text, records, n, offsets=None, before=0, after=0, unit="symbols", merge=True, pos_base=0, n_symbols=None, count=None,
                        gather=True, out=None, out_capacity=None):
        """acm_gpu_context_records_device(): the text round the matches records[:n] (an int64
        [capacity, 2] device tensor; see context_records) of `text` (a device tensor), queued on the
        current stream.  `count` (a device int64 tensor) gives the number of records on the device: n
        is the room of `records` then.  `offsets` is a device int64 tensor of n_texts + 1 entries.
        With gather the snippets are packed into `out` (None: a new uint8 tensor with room for
        out_capacity symbols, by default for the whole buffer; it must not overlap `text`).  Returns a
        Snippets of device tensors; synchronises to read its numbers."""
        import torch
        n_symbols = self._text_args(text, n_symbols)
        assert records.is_cuda and records.is_contiguous() and records.dtype == torch.int64 and records.shape[0] >= int(n)
        n = int(n)
        snip_lo, out_off, snip_text, rec_snip, rec_at, res, out, out_capacity = self._context_outputs(text, n, n_symbols, gather, out, out_capacity)
        off_ptr, n_texts = _cut(offsets)
        tmp = _scratch(lib().acm_gpu_context_tmp_bytes(self.h, n, n_texts), text.device)
        _check(lib().acm_gpu_context_records_device(self.h, text.data_ptr(), n_symbols, pos_base, off_ptr,
                                                    n_texts, records.data_ptr(), n, _opt(count), int(before),
                                                    int(after), _context_flags(unit, merge), _opt(out), out_capacity,
                                                    res.data_ptr() + 16, res.data_ptr() + 8, snip_lo.data_ptr(), out_off.data_ptr(),
                                                    snip_text.data_ptr(), rec_snip.data_ptr(), rec_at.data_ptr(), tmp.data_ptr(), tmp.numel(),
                                                    self._stream()), "acm_gpu_context_records_device")
        _, n_snippets, out_symbols = (int(x) for x in res.cpu())
        return Snippets(out, out_off, snip_lo, snip_text, rec_snip, rec_at, n_snippets, out_symbols, out_capacity, records,
                        int(count.item()) if count is not None else n, self.sym_size)

    def scan_context(self, text, offsets=None, before=0, after=0, unit="symbols", merge=True, n_symbols=None, pos_base=0, capacity=None, records=None,
                     gather=True, out=None, out_capacity=None):
        """acm_gpu_scan_context_device(): the ordered scan of a device tensor and the text round its
        matches (see context_records), queued on the current stream.  `capacity` must hold ALL
        matches.  Returns a Snippets of device tensors whose `records` are the matches in canonical
        order: count > capacity is the number of ALL matches (n_snippets = out_symbols = 0 then);
        out_symbols > out_capacity is the room the output needs.  Synchronises to read the three."""
        n_symbols = self._text_args(text, n_symbols)
        records, cap = self._records_room(records, capacity, n_symbols, text.device)
        snip_lo, out_off, snip_text, rec_snip, rec_at, res, out, out_capacity = self._context_outputs(text, cap, n_symbols, gather, out, out_capacity)
        off_ptr, n_texts = _cut(offsets)
        tmp = _scratch(lib().acm_gpu_scan_context_tmp_bytes(self.h, cap, n_symbols, n_texts), text.device)
        _check(lib().acm_gpu_scan_context_device(self.h, text.data_ptr(), n_symbols, pos_base, off_ptr,
                                                 n_texts, records.data_ptr(), cap, res.data_ptr(), int(before), int(after),
                                                 _context_flags(unit, merge), _opt(out), out_capacity, res.data_ptr() + 16,
                                                 res.data_ptr() + 8, snip_lo.data_ptr(), out_off.data_ptr(), snip_text.data_ptr(),
                                                 rec_snip.data_ptr(), rec_at.data_ptr(), tmp.data_ptr(), tmp.numel(), self._stream()),
               "acm_gpu_scan_context_device")
        count, n_snippets, out_symbols = (int(x) for x in res.cpu())
        return Snippets(out, out_off, snip_lo, snip_text, rec_snip, rec_at, n_snippets, out_symbols, out_capacity, records, count, self.sym_size)

    def scan_context_host(self, text, offsets=None, before=0, after=0, unit="symbols", merge=True, pos_base=0, capacity=None, gather=True,
                          out_capacity=None):
        """acm_gpu_scan_context_host(): numpy in, a Snippets of numpy arrays out, through the C ABI only
        (no torch); each overflow is repeated once with the size the call reports."""
        t = np.ascontiguousarray(text)
        n_sym = t.size * t.itemsize // self.sym_size
        off = np.ascontiguousarray(offsets, dtype=np.uint64) if offsets is not None else None
        call = _context_scan_call(lib().acm_gpu_scan_context_host, (self.h,), t, n_sym, (int(pos_base), *_cut(off)), before, after,
                                  _context_flags(unit, merge))
        return _context_host_call(call, "acm_gpu_scan_context_host", t, self.sym_size, int(capacity) if capacity is not None else max(1024, n_sym // 64),
                                  capacity is None, gather, out_capacity)

    def grep_context_lines(self, buffer, delims=b"\n", before=0, after=0, runs=False, capacity=None, out=None, out_capacity=None):
        """`grep -F -f keywords -C n file` on a device buffer: split() into lines, then scan_context()
        with unit "texts" and merge -- every line with a match with `before` lines in front of it and
        `after` behind it, overlapping and adjacent groups joined as grep joins them -- all on the
        device.  Returns scan_context()'s Snippets with `offsets`, the lines' offsets, beside: snippet
        j is one group, snip_text[j] the number of its first line."""
        offsets = self.split(buffer, delims, runs)
        s = self.scan_context(buffer, offsets, before, after, "texts", True, capacity=capacity, out=out, out_capacity=out_capacity)
        s.offsets = offsets
        return s

    def _replace_inputs(self, text, n_symbols, replacements, fill, out, out_capacity, most_records):
        import torch
        n_symbols = self._text_args(text, n_symbols)
        data, off, nk = replacement_table(replacements, self.sym_size, fill)
        d_data = torch.from_numpy(data.view(np.uint8).copy()).to(text.device)
        d_off = torch.from_numpy(off.view(np.int64).copy()).to(text.device) if off is not None else None
        if out_capacity is None:
            if out is not None:
                out_capacity = out.numel() * out.element_size() // self.sym_size
            else:                                                   # every record grows the text by less than the longest replacement
                longest = int(np.diff(off.astype(np.int64)).max()) if off is not None and nk else 1
                out_capacity = n_symbols + most_records * max(longest - 1, 0)
        if out is None:
            out = torch.empty(max(out_capacity * self.sym_size, 16), dtype=torch.uint8, device=text.device)
        assert out.is_cuda and out.is_contiguous() and out.numel() * out.element_size() >= out_capacity * self.sym_size
        return n_symbols, d_data, d_off, nk, out, int(out_capacity)

    def replace_records(self, text, records, n, replacements=None, fill=None, pos_base=0, n_symbols=None, out=None, out_capacity=None,
                        out_start=False, count=None):
        """acm_gpu_replace_records_device(): `text` (a device tensor) with the selection records[:n] (an
        int64 [capacity, 2] device tensor: canonical order, no two records sharing a symbol) replaced
        by `replacements` (one entry per keyword, see replacement_table) or masked with `fill`, into
        `out` (None: a new uint8 tensor; it must not overlap `text`).  `count` (a device int64 tensor)
        gives the number of records on the device: n is the room of `records` then.  Returns a
        Replaced; synchronises to read out_symbols."""
        import torch
        assert records.is_cuda and records.is_contiguous() and records.dtype == torch.int64 and records.shape[0] >= int(n)
        n = int(n)
        n_symbols, d_data, d_off, nk, out, out_capacity = self._replace_inputs(text, n_symbols, replacements, fill, out, out_capacity, n)
        res = _i64(1, text.device)
        starts = _i64(max(n, 1), text.device) if out_start else None
        tmp = _scratch(lib().acm_gpu_replace_tmp_bytes(self.h, n, n_symbols), text.device)
        _check(lib().acm_gpu_replace_records_device(self.h, text.data_ptr(), n_symbols, pos_base, records.data_ptr(), n, _opt(count), d_data.data_ptr(),
                                                    _opt(d_off), nk, out.data_ptr(), out_capacity, res.data_ptr(), _opt(starts), tmp.data_ptr(),
                                                    tmp.numel(), self._stream()), "acm_gpu_replace_records_device")
        return Replaced(out, int(res.item()), out_capacity, records, int(count.item()) if count is not None else n, starts)

    def scan_replace(self, text, replacements=None, fill=None, n_symbols=None, pos_base=0, capacity=None, records=None, out=None,
                     out_capacity=None, out_start=False):
        """acm_gpu_scan_replace_device(): the ordered scan of a device tensor, the leftmost-longest
        selection of its records and the replacement, queued on the current stream.  `capacity` must
        hold ALL matches.  Returns a Replaced: count > capacity is the number of ALL matches (nothing
        was replaced, out_symbols is 0); out_symbols > out_capacity is the room the output needs.
        Synchronises to read the two."""
        if n_symbols is None:
            n_symbols = text.numel() * text.element_size() // self.sym_size
        records, cap = self._records_room(records, capacity, n_symbols, text.device)
        n_symbols, d_data, d_off, nk, out, out_capacity = self._replace_inputs(text, n_symbols, replacements, fill, out, out_capacity, cap)
        res = _i64(2, text.device)
        starts = _i64(max(cap, 1), text.device) if out_start else None
        tmp = _scratch(lib().acm_gpu_scan_replace_tmp_bytes(self.h, cap, n_symbols), text.device)
        _check(lib().acm_gpu_scan_replace_device(self.h, text.data_ptr(), n_symbols, pos_base, records.data_ptr(), cap, res.data_ptr(),
                                                 d_data.data_ptr(), _opt(d_off), nk, out.data_ptr(), out_capacity, res.data_ptr() + 8, _opt(starts),
                                                 tmp.data_ptr(), tmp.numel(), self._stream()), "acm_gpu_scan_replace_device")
        count, out_symbols = (int(x) for x in res.cpu())
        return Replaced(out, out_symbols, out_capacity, records, count, starts)

    def scan_replace_host(self, text, replacements=None, fill=None, out_capacity=None):
        """acm_gpu_scan_replace_host(): numpy in, (the new text, the number of matches replaced) out,
        through the C ABI only (no torch).  No record capacity: the call counts the matches first.  An
        output overflow is repeated once with the size the call reports when out_capacity is None."""
        return _replace_host_call(lib().acm_gpu_scan_replace_host, "acm_gpu_scan_replace_host", self.h, np.ascontiguousarray(text), self.sym_size,
                                  replacements, fill, out_capacity)

    def _token_outputs(self, dev, token_capacity, n_texts, count_only):
        import torch
        cap = int(token_capacity)
        if count_only:
            ids = start = length = None
        else:
            ids = torch.zeros(max(cap, 1), dtype=torch.int32, device=dev)
            start = _i64(max(cap, 1), dev)
            length = torch.zeros(max(cap, 1), dtype=torch.int32, device=dev)
        first = _i64(n_texts + 1, dev) if n_texts is not None else None
        return cap, ids, start, length, first

    @staticmethod
    def _token_inputs(offsets, tok_of, dev):
        """what the two token calls make of `offsets` (an int64 device tensor of n_texts + 1 entries, or None: one
        text) and tok_of: (the offsets' address, n_texts or None, tok_of on the device or None, its entries)"""
        import torch
        assert offsets is None or (offsets.is_cuda and offsets.is_contiguous() and offsets.dtype == torch.int64)
        off_ptr, n_texts = _cut(offsets)
        table, nk = _tok_of(tok_of)
        d_of = torch.from_numpy(table.view(np.int32).copy()).to(dev) if table is not None else None
        return off_ptr, n_texts if offsets is not None else None, d_of, nk

    def tokens_records(self, text, records, n, offsets=None, mode="run", gap_base=0, tok_of=None, pos_base=0, n_symbols=None, token_capacity=None,
                       count=None, count_only=False):
        """acm_gpu_tokens_records_device(): the token stream of `text` (a device tensor; may be None in
        "run" and "drop" mode with n_symbols given) under the selection records[:n] (an int64
        [capacity, 2] device tensor: canonical order, no two records sharing a symbol).  `offsets` (an
        int64 device tensor of n_texts + 1 entries) makes the buffer a batch; `count` (a device int64
        tensor) gives the number of records on the device, n is the room of `records` then.
        token_capacity: by default n_symbols, which always suffices.  Returns a Tokens of device
        tensors; synchronises to read n_tokens."""
        import torch
        assert records.is_cuda and records.is_contiguous() and records.dtype == torch.int64 and records.shape[0] >= int(n)
        n = int(n)
        dev = records.device
        if n_symbols is None:
            n_symbols = text.numel() * text.element_size() // self.sym_size
        off_ptr, n_texts, d_of, nk = self._token_inputs(offsets, tok_of, dev)
        cap, ids, start, length, first = self._token_outputs(dev, n_symbols if token_capacity is None else token_capacity, n_texts, count_only)
        res = _i64(1, dev)
        tmp = _scratch(lib().acm_gpu_tokens_tmp_bytes(self.h, n, n_symbols), dev)
        _check(lib().acm_gpu_tokens_records_device(self.h, _opt(text), n_symbols, pos_base, records.data_ptr(), n, _opt(count), off_ptr, n_texts or 0,
                                                   _opt(d_of), nk, int(gap_base), _token_mode(mode), _opt(ids), _opt(start), _opt(length), cap,
                                                   res.data_ptr(), _opt(first), tmp.data_ptr(), tmp.numel(), self._stream()),
               "acm_gpu_tokens_records_device")
        return Tokens(ids, start, length, first, int(res.item()), records, int(count.item()) if count is not None else n, cap)

    def scan_tokens(self, text, offsets=None, mode="run", gap_base=0, tok_of=None, n_symbols=None, pos_base=0, capacity=None, records=None,
                    token_capacity=None, count_only=False):
        """acm_gpu_scan_tokens_device(): the ordered scan of a device tensor (with `offsets`, an int64
        device tensor of n_texts + 1 entries: the batch scan, every text from the root on its own), the
        leftmost-longest selection of its records and the token passes, queued on the current stream.
        `capacity` must hold ALL matches of the buffer.  token_capacity: by default n_symbols, which
        always suffices.  Returns a Tokens of device tensors: count > capacity is a record room that
        suffices (n_tokens is 0 then); n_tokens > token_capacity is the room the tokens need.
        Synchronises to read the two."""
        n_symbols = self._text_args(text, n_symbols)
        dev = text.device
        records, cap_r = self._records_room(records, capacity, n_symbols, dev)
        off_ptr, n_texts, d_of, nk = self._token_inputs(offsets, tok_of, dev)
        cap, ids, start, length, first = self._token_outputs(dev, n_symbols if token_capacity is None else token_capacity, n_texts, count_only)
        res = _i64(2, dev)
        tmp = _scratch(lib().acm_gpu_scan_tokens_tmp_bytes(self.h, cap_r, n_symbols, n_texts or 0), dev)
        _check(lib().acm_gpu_scan_tokens_device(self.h, text.data_ptr(), n_symbols, pos_base, off_ptr, n_texts or 0, records.data_ptr(), cap_r,
                                                res.data_ptr(), _opt(d_of), nk, int(gap_base), _token_mode(mode), _opt(ids), _opt(start), _opt(length),
                                                cap, res.data_ptr() + 8, _opt(first), tmp.data_ptr(), tmp.numel(), self._stream()),
               "acm_gpu_scan_tokens_device")
        count, n_tokens = (int(x) for x in res.cpu())
        return Tokens(ids, start, length, first, n_tokens, records, count, cap)

    def scan_tokens_host(self, text, offsets=None, mode="run", gap_base=0, tok_of=None, token_capacity=None):
        """acm_gpu_scan_tokens_host(): numpy in, a Tokens of numpy arrays out, through the C ABI only (no
        torch).  No record capacity: the call counts the matches first.  token_capacity None: the call
        is made twice, count and then fill."""
        off = np.ascontiguousarray(offsets, dtype=np.uint64) if offsets is not None else None
        return _tokenize_host_call(lib().acm_gpu_scan_tokens_host, "acm_gpu_scan_tokens_host", self.h, np.ascontiguousarray(text), self.sym_size, off,
                                   mode, gap_base, tok_of, token_capacity)

    def stream(self, max_piece_symbols, record_capacity):
        return Stream(self, max_piece_symbols, record_capacity)

    def flows(self, n_flows):
        """acm_gpu_flows_create(): the state of n_flows flows (connections, files, log sources) on the
        device, all at the root; Flows.scan() is a batch scan whose texts continue them."""
        return Flows(self, n_flows)

    def wire(self, span, pos_lo):
        """(pos_lo, pos_bits, len_bits) for the 8-byte wire form of the records of a scan of `span` symbols
        with pos_base = pos_lo (acm_gpu_wire_bits), or None when the fields do not fit 64 bits."""
        pb, lb, kb = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        if lib().acm_gpu_wire_bits(self.h, int(span), C.byref(pb), C.byref(lb), C.byref(kb)) != 0:
            return None
        return int(pos_lo), int(pb.value), int(lb.value)

    def status(self):
        """Synchronises and raises if a device-side consistency check failed."""
        _check(lib().acm_gpu_plan_status(self.h), "acm_gpu_plan_status")

    def timing(self, enable=True):
        """True / 1: HIP events around every launch's scan kernel; N > 1: around every N-th launch's; False: off."""
        _check(lib().acm_gpu_plan_timing(self.h, int(enable)), "acm_gpu_plan_timing")

    def timing_read(self):
        ms, n = C.c_double(0), C.c_uint64(0)
        _check(lib().acm_gpu_plan_timing_read(self.h, C.byref(ms), C.byref(n)), "acm_gpu_plan_timing_read")
        return ms.value, int(n.value)

    def timing_read_all(self):
        """(scan kernels' ms, ms from each scan kernel's start to the end of its expansion /
        hole-closing kernel, launches) since timing(True)."""
        ms, allms, n = C.c_double(0), C.c_double(0), C.c_uint64(0)
        _check(lib().acm_gpu_plan_timing_read_all(self.h, C.byref(ms), C.byref(allms), C.byref(n)), "acm_gpu_plan_timing_read_all")
        return ms.value, allms.value, int(n.value)


def pack_records(records, wire):
    """acm_gpu_pack_records_device: int64 [n, 2] CUDA tensor of ordered records -> int64 [n] tensor of 8-byte words."""
    import torch
    pos_lo, pb, lb = wire
    n = records.shape[0]
    out = torch.empty(n, dtype=torch.int64, device=records.device)
    with torch.cuda.device(records.device):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _check(lib().acm_gpu_pack_records_device(records.data_ptr(), n, pos_lo, pb, lb, out.data_ptr(), st), "acm_gpu_pack_records_device")
    return out


def unpack_records(packed, wire, out):
    """acm_gpu_unpack_records_device: int64 [n] CUDA tensor -> the records, into `out` (int64 [n, 2], same device)."""
    import torch
    pos_lo, pb, lb = wire
    assert packed.is_cuda and out.is_cuda and out.shape[0] == packed.shape[0] and out.is_contiguous()
    with torch.cuda.device(out.device):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _check(lib().acm_gpu_unpack_records_device(packed.data_ptr(), packed.shape[0], pos_lo, pb, lb, out.data_ptr(), st), "acm_gpu_unpack_records_device")
    return out


class MultiScan(_Owner):
    """acm_gpu_multi_*: one process, shard r of a text on devices[r] (a device may repeat), the
    ordered records gathered on devices[0] by peer copies -- the C caller's way to use the GPUs of
    a node (include/acm_gpu.h); torch.distributed jobs use sharded.py instead."""

    def __init__(self, machine, devices):
        self.devices = list(devices)
        arr = (C.c_int * len(self.devices))(*self.devices)
        h = C.c_void_p()
        _check(lib().acm_gpu_multi_create(machine.handle, arr, len(self.devices), C.byref(h)), "acm_gpu_multi_create")
        self.h = h

    def close(self):
        if self.h:
            lib().acm_gpu_multi_destroy(self.h)
            self.h = None

    def shard_bounds(self, n_symbols, shard):
        rb, b, e = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().acm_gpu_multi_shard_bounds(self.h, n_symbols, shard, C.byref(rb), C.byref(b), C.byref(e)), "acm_gpu_multi_shard_bounds")
        return int(rb.value), int(b.value), int(e.value)

    def scan_host(self, text, capacity=None):
        """numpy text in host memory -> records of the whole text in canonical order (numpy)."""
        t = np.ascontiguousarray(text)
        n = t.size
        cap = int(capacity) if capacity is not None else max(n // 16, 1024)
        while True:
            out = np.zeros(cap, dtype=RECORD_DTYPE)
            found = C.c_uint64(0)
            rc = lib().acm_gpu_multi_scan_host(self.h, t.ctypes.data, n, out.ctypes.data, cap, C.byref(found))
            if rc == -4 and capacity is None:       # ACM_GPU_E_OVERFLOW: the call says how many there are
                cap = int(found.value)
                continue
            _check(rc, "acm_gpu_multi_scan_host")
            return out[:found.value]

    def scan_device(self, shard_tensors, n_symbols, records):
        """shard_tensors[r]: torch tensor on devices[r] holding [read_begin_r, own_end_r); records:
        int64 [cap, 2] tensor on devices[0].  Returns the number of records (all of the text's)."""
        ptrs = (C.c_void_p * len(shard_tensors))(*[int(t.data_ptr()) for t in shard_tensors])
        found = C.c_uint64(0)
        _check(lib().acm_gpu_multi_scan_device(self.h, ptrs, n_symbols, records.data_ptr(), records.shape[0], C.byref(found)),
               "acm_gpu_multi_scan_device")
        return int(found.value)


class Comm(_Owner):
    """acm_gpu_comm_*: one process (or, in the tests, one thread) per rank; the ranks' ordered
    records gathered on a root over RCCL through the C ABI (include/acm_gpu.h).  `unique_id()` on
    one rank, its 128 bytes handed to the others, then Comm(id, rank, world) on every rank with its
    device current."""

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        _check(lib().acm_gpu_comm_unique_id(buf), "acm_gpu_comm_unique_id")
        return buf.raw

    def __init__(self, unique_id, rank, world, root=0):
        self.rank, self.world, self.root = int(rank), int(world), int(root)
        self.nccl = C.c_void_p()
        self.h = C.c_void_p()
        _check(lib().acm_gpu_comm_init_rank(C.create_string_buffer(bytes(unique_id), 128), self.rank, self.world, C.byref(self.nccl)),
               "acm_gpu_comm_init_rank")
        _check(lib().acm_gpu_comm_create(self.nccl, self.rank, self.world, self.root, C.byref(self.h)), "acm_gpu_comm_create")

    def gather_records(self, plan, local, n_local, pos_lo, span, out=None, stream=None):
        """local: int64 [*, 2] device tensor with this rank's n_local ordered records (positions in
        [pos_lo, pos_lo + span)); out: int64 [cap, 2] device tensor on the root (None elsewhere).
        Returns (records of all ranks, per-rank counts); raises ACMError(-4) on every rank when the
        root's buffer is too small."""
        total = C.c_uint64(0)
        counts = (C.c_uint64 * self.world)()
        rc = lib().acm_gpu_comm_gather_records(self.h, plan.h if plan is not None else None, local.data_ptr() if n_local else None, int(n_local),
                                               int(pos_lo), int(span), out.data_ptr() if out is not None else None,
                                               out.shape[0] if out is not None else 0, C.byref(total), counts, stream)
        if rc == -4:
            raise ACMError(rc, "acm_gpu_comm_gather_records: %d records, more than the root's buffer holds" % total.value)
        _check(rc, "acm_gpu_comm_gather_records")
        return int(total.value), [int(x) for x in counts]

    def close(self):
        if self.h:
            lib().acm_gpu_comm_destroy(self.h)
            self.h = None
        if self.nccl:
            lib().acm_gpu_comm_free(self.nccl)
            self.nccl = None


class Flows(_Owner):
    """acm_gpu_flows_* / acm_gpu_scan_flows_*: a batch scan whose text t continues flow flow[t] -- a
    keyword cut by the boundary between two pieces of a flow is found, with end_pos in the piece it
    ends in.  Results as Plan.scan_batch gives them: numpy arrays (records, text_id, first)."""

    def __init__(self, plan, n_flows):
        self.plan = plan
        self.n_flows = int(n_flows)
        h = C.c_void_p()
        _check(lib().acm_gpu_flows_create(plan.h, self.n_flows, C.byref(h)), "acm_gpu_flows_create")
        self.h = h

    def scan(self, text, offsets, flow=None, capacity=None):
        """acm_gpu_scan_flows_device(): `text` and `offsets` (int64) as in Plan.scan_batch, `flow` an
        int32 device tensor of n_texts flow ids (None: text t is flow t).  An overflow is repeated
        once with the size the call reports (the flows have not moved)."""
        import torch
        p = self.plan
        n_symbols, n_texts = p._batch_args(text, offsets)
        assert flow is None or (flow.is_cuda and flow.is_contiguous() and flow.dtype == torch.int32 and flow.numel() == n_texts)

        def launch(records, text_id, first, cap, count):
            tmp = _scratch(lib().acm_gpu_scan_flows_tmp_bytes(p.h, self.h, cap, n_symbols, n_texts), text.device)
            _check(lib().acm_gpu_scan_flows_device(p.h, self.h, text.data_ptr(), n_symbols, offsets.data_ptr(), _opt(flow), n_texts,
                                                   records.data_ptr(), text_id.data_ptr(), first.data_ptr(), cap, count.data_ptr(), tmp.data_ptr(),
                                                   tmp.numel(), p._stream()), "acm_gpu_scan_flows_device")
        return p._batch_records_device(launch, "acm_gpu_scan_flows_device", text.device, n_texts,
                                       int(capacity) if capacity is not None else max(1024, n_symbols // 64))

    def scan_host(self, text, offsets, flow=None, capacity=None):
        """acm_gpu_scan_flows_host(): the same from host arrays, through the C ABI only (no torch)."""
        p = self.plan
        t = np.ascontiguousarray(text)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        assert off.size >= 1, "offsets has n_texts + 1 entries"
        n_texts = off.size - 1
        fl = None if flow is None else np.ascontiguousarray(flow, dtype=np.uint32)
        assert fl is None or fl.size == n_texts
        n_sym = t.size * t.itemsize // p.sym_size
        return _batch_records_host_call(lib().acm_gpu_scan_flows_host, "acm_gpu_scan_flows_host",
                                        (p.h, self.h, t.ctypes.data, n_sym, off.ctypes.data, _opt(fl), n_texts), n_texts,
                                        int(capacity) if capacity is not None else max(1024, n_sym // 64))

    def reset(self, ids=None):
        """acm_gpu_flows_reset(): the flows `ids` (an int32 device tensor; None: all) back to the root."""
        if ids is not None:
            import torch
            assert ids.is_cuda and ids.is_contiguous() and ids.dtype == torch.int32
        _check(lib().acm_gpu_flows_reset(self.h, _opt(ids), ids.numel() if ids is not None else 0,
                                         self.plan._stream() if ids is not None else None), "acm_gpu_flows_reset")

    def close(self):
        if self.h:
            lib().acm_gpu_flows_destroy(self.h)
            self.h = None


class Stream(_Owner):
    """acm_gpu_stream_*: feed host buffers piece by piece, get the records of the whole stream."""

    def __init__(self, plan, max_piece_symbols, record_capacity):
        self.plan = plan
        self.capacity = int(record_capacity)
        h = C.c_void_p()
        _check(lib().acm_gpu_stream_open(plan.h, int(max_piece_symbols), self.capacity, C.byref(h)), "acm_gpu_stream_open")
        self.h = h
        self._keep = []

    def feed(self, array):
        """array: contiguous numpy array (or anything exposing ctypes.data and nbytes) of symbols"""
        a = np.ascontiguousarray(array)
        self._keep = (self._keep + [a])[-3:]      # the library reads it asynchronously
        n = a.size * a.itemsize // self.plan.sym_size
        _check(lib().acm_gpu_stream_feed(self.h, a.ctypes.data, n), "acm_gpu_stream_feed")

    def feed_ptr(self, ptr, n_symbols):
        _check(lib().acm_gpu_stream_feed(self.h, ptr, int(n_symbols)), "acm_gpu_stream_feed")

    def finish(self):
        out = np.zeros(self.capacity, dtype=RECORD_DTYPE)
        n = C.c_uint64(0)
        _check(lib().acm_gpu_stream_finish(self.h, out.ctypes.data, self.capacity, C.byref(n)), "acm_gpu_stream_finish")
        return out[:n.value]

    def close(self):
        if self.h:
            lib().acm_gpu_stream_close(self.h)
            self.h = None
