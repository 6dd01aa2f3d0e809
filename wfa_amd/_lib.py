"""Loader of libwfahip.so (the HIP hot path).  There is no fallback: if the library is missing the
import of any product entry point fails loudly."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libwfahip.so")

# whole-call codes / per-pair status (include/wfa_hip.h)
OK, ERR_NO_DEVICE, ERR_BAD_ARG, ERR_OOM, ERR_HIP, ERR_UNSUPPORTED, ERR_INTERNAL = 0, -1, -2, -3, -4, -5, -6
PAIR_OK, PAIR_EMPTY, PAIR_TOO_LONG, PAIR_NO_MEMORY = 0, 1, 2, 4
PAIR_OVER_MAX = 8  # the entries that take a max_score: the pair's score exceeds it
PAIR_CHECK_FAILED = 16  # wfahip_check_alignments*'s pass array: an OK pair with a flag of the caller's mask
# wfahip_check_alignments*: the words of a pair's verdict and the bits of its FLAGS word
CHK_WORDS = 8
CHK_W_FLAGS, CHK_W_COST, CHK_W_Q_USED, CHK_W_T_USED, CHK_W_N_BAD, CHK_W_FIRST_BAD = range(6)
CHK_NAMES = ("OPS_RANGE", "LETTER", "ZERO", "UNMERGED", "NO_M", "SEQ_RANGE", "Q_OVER", "Q_UNDER", "T_OVER", "T_UNDER", "M_DIFFERS",
             "X_EQUAL", "NO_ROWS", "NO_ROWS_TRIMMED", "COST_OVER", "COST_UNDER", "STAT_ALIGN_LEN", "STAT_MATCHES", "STAT_GAPS",
             "STAT_GAP_REGIONS")
(CHK_OPS_RANGE, CHK_LETTER, CHK_ZERO, CHK_UNMERGED, CHK_NO_M, CHK_SEQ_RANGE, CHK_Q_OVER, CHK_Q_UNDER, CHK_T_OVER, CHK_T_UNDER,
 CHK_M_DIFFERS, CHK_X_EQUAL, CHK_NO_ROWS, CHK_NO_ROWS_TRIMMED, CHK_COST_OVER, CHK_COST_UNDER, CHK_STAT_ALIGN_LEN, CHK_STAT_MATCHES,
 CHK_STAT_GAPS, CHK_STAT_GAP_REGIONS) = (1 << k for k in range(20))
CHK_ALL = (1 << 20) - 1
# wfahip_pileup*: the counters of a target base (A C T G: the packer's codes)
PILE_WORDS = 8
PILE_W_A, PILE_W_C, PILE_W_T, PILE_W_G, PILE_W_OTHER, PILE_W_GAP, PILE_W_EXTRA, PILE_W_EXTRA_BASES = range(8)
PILE_NAMES = ("A", "C", "T", "G", "OTHER", "GAP", "EXTRA", "EXTRA_BASES")
PILE_MAX_N = (1 << 61) // PILE_WORDS
MAX_SEQ_LEN = (1 << 29) - 1
REC_WORDS = 16
(REC_STATUS, REC_SCORE, REC_TBEGIN, REC_TEND, REC_QBEGIN, REC_QEND, REC_ALIGN_LEN, REC_MATCHES, REC_GAPS,
 REC_GAP_REGIONS, REC_OPS_LEN, REC_OPS_OFF_LO, REC_OPS_OFF_HI, REC_CELLS_LO, REC_CELLS_HI, REC_N_SCORES) = range(16)

# every symbol include/wfa_hip.h declares
EXPORTS = [
    "wfahip_version", "wfahip_strerror", "wfahip_device_count", "wfahip_create", "wfahip_destroy",
    "wfahip_align_batch", "wfahip_results_free", "wfahip_align_batch_device", "wfahip_last_timing",
    "wfahip_set_option", "wfahip_debug_wavefronts", "wfahip_free", "wfahip_gen_stride",
    "wfahip_generate_pairs", "wfahip_packed_words", "wfahip_pack_pairs", "wfahip_align_batch_packed", "wfahip_align_batch_packed_rc", "wfahip_submit",
    "wfahip_pending", "wfahip_collect", "wfahip_create_multi", "wfahip_destroy_multi", "wfahip_multi_size",
    "wfahip_multi_ctx", "wfahip_align_batch_multi", "wfahip_debug_compact_arena",
    "wfahip_generate_pairs_device", "wfahip_align_pair", "wfahip_last_error", "wfahip_debug_clock",
    "wfahip_debug_team_compact", "wfahip_score_batch", "wfahip_scores_free", "wfahip_score_matrix",
    "wfahip_debug_score_long_list", "wfahip_score_batch_device", "wfahip_debug_score_device_list",
    "wfahip_align_batch_bounded", "wfahip_align_batch_bounded_device", "wfahip_score_batch_packed",
    "wfahip_wide_class_bounds", "wfahip_debug_wide_plan", "wfahip_debug_prepack",
    "wfahip_score_batch_packed_rc", "wfahip_score_matrix_rc", "wfahip_revcomp_packed",
    "wfahip_cigar_text_device", "wfahip_cigar_text", "wfahip_cigars_free", "wfahip_align_batch_text",
    "wfahip_alignment_text_device", "wfahip_alignment_text", "wfahip_align_texts_free",
    "wfahip_pack_pairs_device", "wfahip_align_batch_packed_device",
    "wfahip_score_batch_packed_device", "wfahip_select_pairs_device",
    "wfahip_alignment_text_packed_device", "wfahip_alignment_text_packed",
    "wfahip_check_alignments_device", "wfahip_check_alignments_packed_device", "wfahip_check_alignments",
    "wfahip_check_alignments_packed",
    "wfahip_diff_text_device", "wfahip_diff_text_packed_device", "wfahip_diff_text", "wfahip_diff_text_packed",
    "wfahip_pileup_device", "wfahip_pileup_packed_device", "wfahip_pileup", "wfahip_pileup_packed",
]


class Params(C.Structure):
    _fields_ = [("mismatch", C.c_uint32), ("gap_open", C.c_uint32), ("gap_ext", C.c_uint32),
                ("global_alignment", C.c_uint8), ("adaptive", C.c_uint8), ("reserved", C.c_uint8 * 2),
                ("min_wf_len", C.c_uint32), ("max_dist_diff", C.c_uint32), ("cutoff_step", C.c_uint32)]


class Results(C.Structure):
    _fields_ = [("n", C.c_uint64), ("status", C.POINTER(C.c_int32)), ("score", C.POINTER(C.c_uint32)),
                ("tbegin", C.POINTER(C.c_int32)), ("tend", C.POINTER(C.c_int32)),
                ("qbegin", C.POINTER(C.c_int32)), ("qend", C.POINTER(C.c_int32)),
                ("align_len", C.POINTER(C.c_uint32)), ("matches", C.POINTER(C.c_uint32)),
                ("gaps", C.POINTER(C.c_uint32)), ("gap_regions", C.POINTER(C.c_uint32)),
                ("ops_off", C.POINTER(C.c_uint64)), ("ops_len", C.POINTER(C.c_uint32)),
                ("ops", C.POINTER(C.c_uint64)), ("n_ops", C.c_uint64)]


class Scores(C.Structure):
    _fields_ = [("n", C.c_uint64), ("status", C.POINTER(C.c_int32)), ("score", C.POINTER(C.c_uint32))]


class Cigars(C.Structure):
    """wfahip_cigars: pair i's CIGAR text is text[off[i] .. off[i + 1])"""
    _fields_ = [("n", C.c_uint64), ("n_bytes", C.c_uint64), ("text", C.POINTER(C.c_uint8)), ("off", C.POINTER(C.c_uint64))]


class AlignTexts(C.Structure):
    """wfahip_align_texts: pair i's rows are q_row, a_row and t_row[off[i] .. off[i + 1])"""
    _fields_ = [("n", C.c_uint64), ("n_bytes", C.c_uint64), ("q_row", C.POINTER(C.c_uint8)), ("a_row", C.POINTER(C.c_uint8)),
                ("t_row", C.POINTER(C.c_uint8)), ("off", C.POINTER(C.c_uint64))]


class Timing(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("total_ms", C.c_double), ("n_launches", C.c_uint32),
                ("n_retried_pairs", C.c_uint32), ("cells_stored", C.c_uint64), ("ops_written", C.c_uint64),
                ("arena_bytes", C.c_uint64), ("main_kernel_ms", C.c_double), ("n_main_launches", C.c_uint32),
                ("n_packed_pairs", C.c_uint32), ("main_kernel_kind", C.c_uint32), ("ladder_start_level", C.c_uint32)]


class Row(C.Structure):
    _fields_ = [("score", C.c_uint32), ("lo", C.c_int32), ("width", C.c_uint32), ("word_off", C.c_uint64)]


_lib = None


def lib():
    """The loaded C-ABI library.  Raises if it has not been built (make, or __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build the HIP extension first "
                               "(`make` or `python -c 'import __graft_entry__ as g; g.build()'`). "
                               "There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        L.wfahip_version.restype = C.c_int
        L.wfahip_strerror.restype = C.c_char_p
        L.wfahip_strerror.argtypes = [C.c_int]
        L.wfahip_device_count.restype = C.c_int
        L.wfahip_create.restype = C.c_int
        L.wfahip_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.wfahip_destroy.argtypes = [vp]
        L.wfahip_align_batch.restype = C.c_int
        L.wfahip_align_batch.argtypes = [vp, C.POINTER(Params), vp, u64, vp, vp, vp, vp, u64, C.POINTER(Results)]
        L.wfahip_results_free.argtypes = [C.POINTER(Results)]
        L.wfahip_score_batch.restype = C.c_int
        L.wfahip_score_batch.argtypes = [vp, C.POINTER(Params), vp, u64, vp, vp, vp, vp, u64, u32, C.POINTER(Scores)]
        L.wfahip_scores_free.argtypes = [C.POINTER(Scores)]
        L.wfahip_score_batch_packed.restype = C.c_int
        L.wfahip_score_batch_packed.argtypes = [vp, C.POINTER(Params), vp, u64, vp, vp, vp, vp, u64, u32, C.POINTER(Scores)]
        L.wfahip_score_batch_packed_rc.restype = C.c_int
        L.wfahip_score_batch_packed_rc.argtypes = [vp, C.POINTER(Params), vp, u64, vp, vp, vp, vp, vp, u64, u32, C.POINTER(Scores)]
        L.wfahip_score_matrix_rc.restype = C.c_int
        L.wfahip_score_matrix_rc.argtypes = [vp, C.POINTER(Params), vp, u64, vp, vp, u64, vp, vp, vp, u64, u32, vp, vp, u64]
        L.wfahip_revcomp_packed.restype = C.c_int
        L.wfahip_revcomp_packed.argtypes = [vp, u32, vp]
        L.wfahip_score_matrix.restype = C.c_int
        L.wfahip_score_matrix.argtypes = [vp, C.POINTER(Params), vp, u64, vp, vp, u64, vp, vp, u64, u32, vp, vp, u64]
        L.wfahip_debug_score_long_list.restype = C.c_int
        L.wfahip_debug_score_long_list.argtypes = [vp, vp, vp, vp, vp, u64, C.POINTER(C.POINTER(u32)), C.POINTER(u64),
                                                   C.POINTER(C.POINTER(u32)), C.POINTER(u64)]
        L.wfahip_score_batch_device.restype = C.c_int
        L.wfahip_score_batch_device.argtypes = [vp, C.POINTER(Params), vp, u64, vp, vp, vp, vp, u64, u32, u32, vp, vp, vp]
        L.wfahip_debug_score_device_list.restype = C.c_int
        L.wfahip_debug_score_device_list.argtypes = [vp, C.POINTER(C.POINTER(u32)), C.POINTER(u64), C.POINTER(C.POINTER(u32)),
                                                     C.POINTER(u64)]
        L.wfahip_wide_class_bounds.restype = C.c_int
        L.wfahip_wide_class_bounds.argtypes = [C.POINTER(u32), C.c_int]
        L.wfahip_debug_wide_plan.restype = C.c_int
        L.wfahip_debug_wide_plan.argtypes = [vp, vp, vp, u64, C.POINTER(C.POINTER(u32)), C.POINTER(u64), C.POINTER(u32),
                                             C.POINTER(u64)]
        L.wfahip_debug_prepack.restype = C.c_int
        L.wfahip_debug_prepack.argtypes = [vp, vp, vp, vp, vp, vp, vp, u64, u32, u32, vp]
        L.wfahip_align_batch_device.restype = C.c_int
        L.wfahip_align_batch_device.argtypes = [vp, C.POINTER(Params), vp, u64, vp, vp, vp, vp, u64, u32, vp, vp,
                                                u64, C.POINTER(u64), vp]
        L.wfahip_align_batch_bounded.restype = C.c_int
        L.wfahip_align_batch_bounded.argtypes = [vp, C.POINTER(Params), vp, u64, vp, vp, vp, vp, u64, u32, C.POINTER(Results)]
        L.wfahip_align_batch_bounded_device.restype = C.c_int
        L.wfahip_align_batch_bounded_device.argtypes = [vp, C.POINTER(Params), vp, u64, vp, vp, vp, vp, u64, u32, u32, vp, vp,
                                                        u64, C.POINTER(u64), vp]
        L.wfahip_cigar_text_device.restype = C.c_int
        L.wfahip_cigar_text_device.argtypes = [vp, vp, vp, u64, u64, C.c_int, vp, u64, vp, C.POINTER(u64), vp]
        L.wfahip_cigar_text.restype = C.c_int
        L.wfahip_cigar_text.argtypes = [C.POINTER(Results), C.c_int, C.c_int, C.POINTER(Cigars)]
        L.wfahip_cigars_free.argtypes = [C.POINTER(Cigars)]
        L.wfahip_align_batch_text.restype = C.c_int
        L.wfahip_align_batch_text.argtypes = [vp, C.POINTER(Params), vp, u64, vp, vp, vp, vp, u64, C.c_int, C.POINTER(Results),
                                              C.POINTER(Cigars)]
        L.wfahip_alignment_text_device.restype = C.c_int
        L.wfahip_alignment_text_device.argtypes = [vp, vp, vp, u64, vp, u64, vp, vp, vp, vp, u64, C.c_int, vp, vp, vp, u64, vp,
                                                   C.POINTER(u64), vp]
        L.wfahip_alignment_text.restype = C.c_int
        L.wfahip_alignment_text.argtypes = [C.POINTER(Results), vp, u64, vp, vp, vp, vp, C.c_int, C.c_int, C.POINTER(AlignTexts)]
        L.wfahip_align_texts_free.argtypes = [C.POINTER(AlignTexts)]
        L.wfahip_alignment_text_packed_device.restype = C.c_int
        L.wfahip_alignment_text_packed_device.argtypes = [vp, vp, vp, u64, vp, u64, vp, vp, vp, vp, vp, u64, C.c_int, vp, vp, vp, u64, vp,
                                                          C.POINTER(u64), vp]
        L.wfahip_alignment_text_packed.restype = C.c_int
        L.wfahip_alignment_text_packed.argtypes = [C.POINTER(Results), vp, u64, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.POINTER(AlignTexts)]
        L.wfahip_check_alignments_device.restype = C.c_int
        L.wfahip_check_alignments_device.argtypes = [vp, C.POINTER(Params), vp, vp, u64, vp, u64, vp, vp, vp, vp, u64, u32, vp, vp,
                                                     C.POINTER(u64), vp]
        L.wfahip_check_alignments_packed_device.restype = C.c_int
        L.wfahip_check_alignments_packed_device.argtypes = [vp, C.POINTER(Params), vp, vp, u64, vp, u64, vp, vp, vp, vp, vp, u64, u32, vp, vp,
                                                            C.POINTER(u64), vp]
        L.wfahip_check_alignments.restype = C.c_int
        L.wfahip_check_alignments.argtypes = [C.POINTER(Results), C.POINTER(Params), vp, u64, vp, vp, vp, vp, u32, C.c_int, vp, vp,
                                              C.POINTER(u64)]
        L.wfahip_check_alignments_packed.restype = C.c_int
        L.wfahip_check_alignments_packed.argtypes = [C.POINTER(Results), C.POINTER(Params), vp, u64, vp, vp, vp, vp, vp, u32, C.c_int, vp, vp,
                                                     C.POINTER(u64)]
        L.wfahip_diff_text_device.restype = C.c_int
        L.wfahip_diff_text_device.argtypes = [vp, vp, vp, u64, vp, u64, vp, vp, vp, vp, u64, C.c_int, vp, u64, vp, C.POINTER(u64), vp]
        L.wfahip_diff_text_packed_device.restype = C.c_int
        L.wfahip_diff_text_packed_device.argtypes = [vp, vp, vp, u64, vp, u64, vp, vp, vp, vp, vp, u64, C.c_int, vp, u64, vp, C.POINTER(u64),
                                                     vp]
        L.wfahip_diff_text.restype = C.c_int
        L.wfahip_diff_text.argtypes = [C.POINTER(Results), vp, u64, vp, vp, vp, vp, C.c_int, C.c_int, C.POINTER(Cigars)]
        L.wfahip_diff_text_packed.restype = C.c_int
        L.wfahip_diff_text_packed.argtypes = [C.POINTER(Results), vp, u64, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.POINTER(Cigars)]
        L.wfahip_pileup_device.restype = C.c_int
        L.wfahip_pileup_device.argtypes = [vp, vp, vp, u64, vp, u64, vp, vp, vp, vp, u64, C.c_int, u64, u64, vp, C.POINTER(u64), vp]
        L.wfahip_pileup_packed_device.restype = C.c_int
        L.wfahip_pileup_packed_device.argtypes = [vp, vp, vp, u64, vp, u64, vp, vp, vp, vp, vp, u64, C.c_int, u64, u64, vp, C.POINTER(u64), vp]
        L.wfahip_pileup.restype = C.c_int
        L.wfahip_pileup.argtypes = [C.POINTER(Results), vp, u64, vp, vp, vp, vp, C.c_int, C.c_int, u64, u64, vp, C.POINTER(u64)]
        L.wfahip_pileup_packed.restype = C.c_int
        L.wfahip_pileup_packed.argtypes = [C.POINTER(Results), vp, u64, vp, vp, vp, vp, vp, C.c_int, C.c_int, u64, u64, vp, C.POINTER(u64)]
        L.wfahip_last_timing.restype = C.c_int
        L.wfahip_last_timing.argtypes = [vp, C.POINTER(Timing)]
        L.wfahip_set_option.restype = C.c_int
        L.wfahip_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
        L.wfahip_debug_wavefronts.restype = C.c_int
        L.wfahip_debug_wavefronts.argtypes = [vp, C.POINTER(Params), C.c_char_p, u32, C.c_char_p, u32,
                                              C.POINTER(C.POINTER(Row)), C.POINTER(u64),
                                              C.POINTER(C.POINTER(u32)), C.POINTER(u64), C.POINTER(Results)]
        L.wfahip_debug_team_compact.restype = C.c_int
        L.wfahip_debug_team_compact.argtypes = [vp, C.POINTER(Params), C.c_char_p, u32, C.c_char_p, u32,
                                              C.POINTER(C.POINTER(Row)), C.POINTER(u64),
                                              C.POINTER(C.POINTER(u32)), C.POINTER(u64), C.POINTER(Results)]
        L.wfahip_free.argtypes = [vp]
        L.wfahip_gen_stride.restype = u64
        L.wfahip_gen_stride.argtypes = [u32, C.c_double]
        L.wfahip_generate_pairs.restype = C.c_int
        L.wfahip_generate_pairs.argtypes = [u64, u64, u64, u32, C.c_double, C.c_int, vp, vp, vp, vp, vp]
        L.wfahip_packed_words.restype = u64
        L.wfahip_packed_words.argtypes = [u32]
        L.wfahip_pack_pairs.restype = C.c_int
        L.wfahip_pack_pairs.argtypes = [vp, vp, vp, vp, vp, u64, C.c_int, vp, vp, vp, C.POINTER(u64)]
        L.wfahip_align_batch_packed.restype = C.c_int
        L.wfahip_align_batch_packed.argtypes = [vp, C.POINTER(Params), vp, u64, vp, vp, vp, vp, u64, C.POINTER(Results)]
        L.wfahip_align_batch_packed_rc.restype = C.c_int
        L.wfahip_align_batch_packed_rc.argtypes = [vp, C.POINTER(Params), vp, u64, vp, vp, vp, vp, vp, u64, C.POINTER(Results)]
        L.wfahip_pack_pairs_device.restype = C.c_int
        L.wfahip_pack_pairs_device.argtypes = [vp, vp, u64, vp, vp, vp, vp, u64, vp, u64, vp, vp, C.POINTER(u64), vp]
        L.wfahip_align_batch_packed_device.restype = C.c_int
        L.wfahip_align_batch_packed_device.argtypes = [vp, C.POINTER(Params), vp, u64, vp, vp, vp, vp, vp, u64, u32, u32, vp, vp,
                                                       u64, C.POINTER(u64), vp]
        L.wfahip_score_batch_packed_device.restype = C.c_int
        L.wfahip_score_batch_packed_device.argtypes = [vp, C.POINTER(Params), vp, u64, vp, vp, vp, vp, vp, u64, u32, u32, vp, vp, vp]
        L.wfahip_select_pairs_device.restype = C.c_int
        L.wfahip_select_pairs_device.argtypes = [vp, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(u64), vp]
        L.wfahip_submit.restype = C.c_int
        L.wfahip_submit.argtypes = [vp, C.c_char_p, u32, C.c_char_p, u32, C.POINTER(u64)]
        L.wfahip_pending.restype = u64
        L.wfahip_debug_clock.restype = C.c_int
        L.wfahip_debug_clock.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.wfahip_align_pair.restype = C.c_int
        L.wfahip_align_pair.argtypes = [vp, C.POINTER(Params), C.c_char_p, u32, C.c_char_p, u32, vp, vp, u64, C.POINTER(u64)]
        L.wfahip_last_error.restype = C.c_char_p
        L.wfahip_last_error.argtypes = [vp]
        L.wfahip_pending.argtypes = [vp]
        L.wfahip_collect.restype = C.c_int
        L.wfahip_collect.argtypes = [vp, C.POINTER(Params), C.POINTER(Results)]
        L.wfahip_create_multi.restype = C.c_int
        L.wfahip_create_multi.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
        L.wfahip_destroy_multi.argtypes = [vp]
        L.wfahip_multi_size.restype = C.c_int
        L.wfahip_multi_size.argtypes = [vp]
        L.wfahip_multi_ctx.restype = vp
        L.wfahip_multi_ctx.argtypes = [vp, C.c_int]
        L.wfahip_align_batch_multi.restype = C.c_int
        L.wfahip_align_batch_multi.argtypes = [vp, C.POINTER(Params), vp, u64, vp, vp, vp, vp, u64, C.POINTER(Results)]
        L.wfahip_debug_compact_arena.restype = C.c_int
        L.wfahip_debug_compact_arena.argtypes = [vp, u64, C.POINTER(C.POINTER(u32)), C.POINTER(u64), C.POINTER(u32),
                                                 C.POINTER(u32 * 4)]
        L.wfahip_generate_pairs_device.restype = C.c_int
        L.wfahip_generate_pairs_device.argtypes = [vp, u64, u64, u64, u32, C.c_double, vp, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


class WfaHipError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        self.code = code
        msg = lib().wfahip_strerror(code).decode()
        super().__init__(f"{what}: {msg} ({code})" if what else f"{msg} ({code})")


def check(code: int, what: str = ""):
    if code != OK:
        raise WfaHipError(code, what)
