"""wfa_amd -- MI355X (gfx950) wavefront alignment behind the shenwei356/wfa Aligner API.

The package holds only what the hot path needs: csrc/ (HIP kernels + the C-ABI of include/wfa_hip.h),
lib/ (the built libwfahip.so) and aligner.py (host-side mirror of the reference's Go API over ctypes).
"""
from .aligner import (  # noqa: F401
    AdaptiveReductionOption, Aligner, AlignmentResult, MultiAligner, pack_pairs, generate_pairs_device, BatchResult, DefaultAdaptiveOption, DefaultOptions,
    DefaultPenalties, ErrEmptySeq, ErrOverMaxScore, ErrSeqTooLong, MaskLower32, MaxSeqLen, New, Op, OpD, OpH, OpI, OpM, OpX,
    Options, Penalties, RecycleAligner, RecycleAlignmentResult, RecycleAlignmentText, WfaError, generate_pairs,
    make_blob, plot_component, trimOps, wide_class_bounds, revcomp_packed, best_strand, cigar_text, alignment_text,
    alignment_text_packed, check_alignments, check_alignments_packed, diff_text, diff_text_packed, pileup, pileup_packed,
)
from ._lib import (  # noqa: F401
    PAIR_CHECK_FAILED, CHK_WORDS, CHK_NAMES, CHK_ALL, CHK_OPS_RANGE, CHK_LETTER, CHK_ZERO, CHK_UNMERGED, CHK_NO_M, CHK_SEQ_RANGE, CHK_Q_OVER,
    CHK_Q_UNDER, CHK_T_OVER, CHK_T_UNDER, CHK_M_DIFFERS, CHK_X_EQUAL, CHK_NO_ROWS, CHK_NO_ROWS_TRIMMED, CHK_COST_OVER, CHK_COST_UNDER,
    CHK_STAT_ALIGN_LEN, CHK_STAT_MATCHES, CHK_STAT_GAPS, CHK_STAT_GAP_REGIONS,
    PILE_WORDS, PILE_NAMES, PILE_W_A, PILE_W_C, PILE_W_T, PILE_W_G, PILE_W_OTHER, PILE_W_GAP, PILE_W_EXTRA, PILE_W_EXTRA_BASES,
)
