/*
 * wfa_hip.h -- C-ABI of libwfahip.so: the MI355X (gfx950) wavefront-alignment hot path behind
 * the shenwei356/wfa Aligner API.
 *
 * Every entry point is `extern "C"`, takes plain pointers and sizes, and is what a cgo binding of
 * the reference's Go package would call in place of its pure-Go path (INTEGRATION.md shows the
 * binding).  Citations are file:line into the reference checkout.
 *
 *   reference interface (Go)                                    replaced by
 *   ----------------------------------------------------------  ---------------------------------
 *   wfa.New(p *Penalties, opt *Options)            wfa.go:120    wfahip_create + wfahip_params
 *   (*Aligner).AdaptiveReduction(ad)               wfa.go:134    wfahip_params.adaptive/min_wf_len/...
 *   (*Aligner).Align / AlignPointers(q, t)         wfa.go:196,201  wfahip_align_batch (n_pairs = 1 or N)
 *   ErrEmptySeq / ErrSeqTooLong / MaxSeqLen        wfa.go:186-193  per-pair status WFAHIP_PAIR_EMPTY / _TOO_LONG
 *   AlignmentResult{Ops,Score,TBegin,...}          wfa_cigar.go:30-48  wfahip_results (struct of arrays)
 *   RecycleAlignmentResult                         wfa_cigar.go:92   wfahip_results_free
 *   RecycleAligner                                 wfa.go:102    wfahip_destroy
 *
 * Threading: one wfahip_ctx may be used by one thread at a time; different contexts may be used
 * concurrently (mirrors "one Aligner per goroutine", wfa.go:73-78).
 *
 * First call of a workload: a context allocates its device buffers on demand and keeps them -- wavefront arenas sized
 * for the batch (34 KB per 1 kbp pair: 32 GiB for a million pairs), staging buffers, the page-locked blocks of the
 * host entry.  hipMalloc of tens of GB and hipHostMalloc of hundreds of MB take SECONDS (2.5-4 s measured for the first
 * 1e6 x 1 kbp call of a context against 20-60 ms for every later one), so a service should align one batch of its
 * largest expected shape right after wfahip_create, before it takes traffic; later calls of the same or a smaller shape
 * allocate nothing.  A context also LEARNS per class of batches (length bucket, penalties, wf-adaptive): the arena level
 * long pairs need, the rows per pair and the window width that high-error batches need.  What is learned changes only
 * how fast a call is, never its results (options "learn", and the tests of it, say how).
 *
 * Results are owned by the library: every array of a wfahip_results is handed back through wfahip_results_free, never
 * free()d by the caller (blocks circulate through a cache and are page-locked while they do).
 */
#ifndef WFA_HIP_H
#define WFA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WFAHIP_VERSION 400 /* 0.4.0 */

/* whole-call return codes (0 = success, negative = failure) */
enum {
    WFAHIP_OK              = 0,
    WFAHIP_ERR_NO_DEVICE   = -1,
    WFAHIP_ERR_BAD_ARG     = -2,
    WFAHIP_ERR_OOM         = -3,
    WFAHIP_ERR_HIP         = -4,
    WFAHIP_ERR_UNSUPPORTED = -5, /* mismatch == 0 or gap_open + gap_ext == 0 (the reference's own backtrace does not
                                    terminate for mismatch == 0 when first bases differ, and next() would read the row it is writing);
                                    non-ACGT input to the packer */
    WFAHIP_ERR_INTERNAL    = -6
};

/* per-pair status (wfahip_results.status) */
enum {
    WFAHIP_PAIR_OK        = 0,
    WFAHIP_PAIR_EMPTY     = 1, /* ErrEmptySeq,   wfa.go:204-206 */
    WFAHIP_PAIR_TOO_LONG  = 2, /* ErrSeqTooLong, wfa.go:207-209 */
    WFAHIP_PAIR_NO_MEMORY = 4, /* wavefront arena could not be grown enough for this pair */
    WFAHIP_PAIR_OVER_MAX  = 8, /* the entries that take a max_score (score entries, wfahip_align_batch_bounded): the pair's score exceeds it */
    WFAHIP_PAIR_CHECK_FAILED = 16 /* wfahip_check_alignments*'s pass array only: an OK pair with a flag of the caller's mask */
};

/* wfa.go:190 MaxSeqLen */
#define WFAHIP_MAX_SEQ_LEN ((1u << 29) - 1u)

/* Penalties (wfa.go:32-36) + Options (wfa.go:64-66) + AdaptiveReductionOption (wfa.go:46-50) */
typedef struct {
    uint32_t mismatch, gap_open, gap_ext;
    uint8_t  global_alignment; /* Options.GlobalAlignment */
    uint8_t  adaptive;         /* 0: AdaptiveReduction was never called (algn.ad == nil) */
    uint8_t  reserved[2];
    uint32_t min_wf_len, max_dist_diff, cutoff_step; /* cutoff_step is unused by the reference too (wfa.go:49) */
} wfahip_params;

/* AlignmentResult as a struct of arrays, one element per pair (wfa_cigar.go:30-48).
 * ops holds, for pair i, ops_len[i] entries starting at ops[ops_off[i]], each `op<<32 | n`
 * (wfa_cigar.go:118-124), already reversed and merged the way AlignmentResult.process() leaves
 * them (wfa_cigar.go:136-214).  All arrays are malloc'd by the library. */
typedef struct {
    uint64_t  n;
    int32_t  *status;
    uint32_t *score;
    int32_t  *tbegin, *tend, *qbegin, *qend;
    uint32_t *align_len, *matches, *gaps, *gap_regions;
    uint64_t *ops_off;
    uint32_t *ops_len;
    uint64_t *ops;
    uint64_t  n_ops;
} wfahip_results;

/* device-side result record: 16 x u32 per pair, one 64-byte line */
enum {
    WFAHIP_REC_STATUS = 0, WFAHIP_REC_SCORE, WFAHIP_REC_TBEGIN, WFAHIP_REC_TEND, WFAHIP_REC_QBEGIN,
    WFAHIP_REC_QEND, WFAHIP_REC_ALIGN_LEN, WFAHIP_REC_MATCHES, WFAHIP_REC_GAPS, WFAHIP_REC_GAP_REGIONS,
    WFAHIP_REC_OPS_LEN, WFAHIP_REC_OPS_OFF_LO, WFAHIP_REC_OPS_OFF_HI,
    WFAHIP_REC_CELLS_LO, WFAHIP_REC_CELLS_HI, /* non-zero wavefront words stored (M+I+D); 0 unless option "census" is on */
    WFAHIP_REC_N_SCORES,
    WFAHIP_REC_WORDS = 16
};

/* timing / accounting of the most recent wfahip_align_batch* call on a context */
typedef struct {
    double   kernel_ms;        /* sum of the alignment kernels' durations (hipEvent, on their stream) */
    double   total_ms;         /* whole device-side call: first launch -> last kernel done */
    uint32_t n_launches;       /* alignment kernel launches (1 + retries for bigger arenas / byte path) */
    uint32_t n_retried_pairs;  /* pairs that needed a second configuration */
    uint64_t cells_stored;     /* sum over pairs of non-zero wavefront words stored */
    uint64_t ops_written;      /* CIGAR ops written */
    uint64_t arena_bytes;      /* arena footprint allocated */
    double   main_kernel_ms;   /* total duration of the dominant kernel's launches (packed forward kernel when it
                                  ran, else the first generic launch) */
    uint32_t n_main_launches;  /* launches of that kernel (one per chunk) */
    uint32_t n_packed_pairs;   /* pairs finished by the sub-wave forward + backtrace kernels */
    uint32_t main_kernel_kind; /* (the library's names for these numbers: enum Kind, wfa_amd/csrc/wfa_kinds.hpp) 0 = wfa_generic_kernel, 1 = wfa_packed_kernel, 2 = wfa_reg_kernel, 3 = wfa_blk_kernel<16>, 4 = wfa_blk_kernel<8>,
                                  5 = wfa_blk_kernel<64>, 6 = wfa_blk_kernel<8, 8, false, 4> (short reads), 7 = wfa_team_kernel,
                                  8 = wfa_duo_kernel (8 or 16 lanes per pair), 9 = wfa_blk_kernel<32> (128 diagonals),
                                  10 = wfa_lane_kernel (a lane per pair, short reads), 11 / 12 / 13 = wfa_blk_kernel<16 / 32 / 64, .., LONG>
                                  (sliding sequence windows: reads of any length, 64 / 128 / 256 diagonals), 14 / 15 = wfa_blk_kernel<64, 1, false, 1 / 2, .., LONG>
                                  (a wave per pair, one / two diagonals per lane: batches too small to fill the GPU),
                                  16 = wfa_blk_kernel<64, 1, false, 1, false, false> (wfahip_align_pair: one launch, forward pass and backtrace),
                                  18 = wfa_wide_kernel (round 6: semi-global reads up to 2 047 bases, a workgroup per pair with the rows in 16-bit LDS rings;
                                  reported whenever one of its launches ran -- a batch of mixed lengths is one launch per length class, and its reads
                                  beyond 2 047 bases take the ladder: n_packed_pairs = pairs it finished, n_retried_pairs = all the others,
                                  main_kernel_ms / n_main_launches summed over the classes, arena_bytes the largest class's),
                                  17 = wfa_teamc_kernel (wide wavefronts: a team of workgroups per pair, one backtrace word per diagonal),
                                  19 = wfa_score_kernel (wfahip_score_batch, global pairs), 20 = wfa_wide_kernel<.., SCORE> (wfahip_score_batch,
                                  semi-global pairs), 21 = wfa_score_kernel<MATRIX> (wfahip_score_matrix, global alignment),
                                  22 = wfa_wide_kernel<.., SCORE, MATRIX> (wfahip_score_matrix, semi-global alignment),
                                  23 = wfa_score_long_kernel (wfahip_score_batch, global pairs of reads beyond 2 047 bases: reported when it took more
                                  pairs of the call than wfa_score_kernel), 24 = wfa_score_long_kernel<MATRIX> (wfahip_score_matrix, likewise by cells) */
    uint32_t ladder_start_level; /* arena level the long-pair ladder of this call started on (0 unless a learned hint applied) */
} wfahip_timing;

typedef struct wfahip_ctx wfahip_ctx;

int         wfahip_version(void);
const char *wfahip_strerror(int code);
/* detail of the most recent WFAHIP_ERR_HIP / WFAHIP_ERR_OOM / WFAHIP_ERR_INTERNAL on a context (the failing runtime call and its
 * message; "" if none): for logs -- the code is what a binding acts on.  Valid until the next call on the context. */
const char *wfahip_last_error(const wfahip_ctx *ctx);
int         wfahip_device_count(void);

/* One context per GPU (one process per GPU in multi-GPU jobs).  device_id < 0 = current device. */
int  wfahip_create(int device_id, wfahip_ctx **out);
void wfahip_destroy(wfahip_ctx *ctx);

/* The cgo entry: host inputs, host outputs, synchronous.  seq_blob holds all sequences; pair i is
 * query seq_blob[q_off[i] .. +q_len[i]) vs target seq_blob[t_off[i] .. +t_len[i]).  Inputs are
 * borrowed for the duration of the call only.  out is filled with malloc'd arrays; release with
 * wfahip_results_free, which keeps the large blocks for the next call (RecycleAlignmentResult,
 * wfa_cigar.go:92: fresh pages cost more than the download).  Replaces Aligner.Align (wfa.go:196).
 * Batches of >= 200 000 pairs whose pairs lie in order in the blob are aligned in four slices while the rest of
 * the blob is still uploading and the results of earlier slices are already downloading.  Environment (diagnostics): WFAHIP_NO_UPLOAD_OVERLAP=1 switches that off,
 * WFAHIP_DL_THREADS=n sets the number of copy-out threads of the result download, WFAHIP_DEBUG_TIMING=1 prints
 * the phases of a call to stderr. */
int  wfahip_align_batch(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *seq_blob,
                        uint64_t blob_bytes, const uint64_t *q_off, const uint32_t *q_len,
                        const uint64_t *t_off, const uint32_t *t_len, uint64_t n_pairs,
                        wfahip_results *out);
void wfahip_results_free(wfahip_results *r);

/* Score only: the AlignmentResult.Score of every pair (wfa_cigar.go:30-48, set from the forward pass at wfa.go:714) without
 * the CIGAR, the match region or the statistics -- WFA2-lib's "score only" alignment scope.  Inputs as wfahip_align_batch.
 * For every pair, status and score equal what wfahip_align_batch returns for the same pair and params (score 0 unless
 * status is WFAHIP_PAIR_OK), global or semi-global, with wf-adaptive on or off, any penalties that entry takes, any bytes.
 * max_score (0 = no bound): a pair whose score would exceed it stops as soon as the score step passes it and gets
 * WFAHIP_PAIR_OVER_MAX -- exactly: global pairs when no M[s][m - n] reached the end by s = max_score, semi-global pairs when no
 * row up to max_score held an end cell (wfa.go:270-375) and none terminated.  Whole-call errors are those of wfahip_align_batch.
 * Only the forward pass runs, with the last rows on chip: no wavefront arena is allocated, nothing is kept for a backtrace.
 * Global pairs with e / g == 1 and x / g, (o+e) / g up to 7 (g = gcd(x, o+e, e)): reads up to 2 047 bases run on
 * wfa_score_kernel; longer reads, up to WFAHIP_MAX_SEQ_LEN, run on wfa_score_long_kernel (32-bit offsets, the sequences read 2-bit
 * packed from global memory through sliding windows) when the call holds at least 64 such pairs (DEBUG option "score_long_min") --
 * fewer take the full path.  Semi-global pairs up to 2 047 bases of the shapes wfahip_align_pair lists run on the score instances of
 * wfa_wide_kernel.  Every other pair -- a shape without an instance, a byte outside ACGT, a longer semi-global read, a band wider
 * than the kernels' 248 diagonals -- is aligned by the full path of wfahip_align_batch and only its score kept.  wfahip_last_timing:
 * main_kernel_kind 19 (wfa_score_kernel), 23 (wfa_score_long_kernel, when it took more pairs of the call than wfa_score_kernel) or
 * 20 (wfa_wide_kernel, score instances), n_retried_pairs = pairs that took the full path, arena_bytes = 0 unless some did.  Release
 * out with wfahip_scores_free (the arrays are malloc'd). */
typedef struct {
    uint64_t  n;
    int32_t  *status; /* WFAHIP_PAIR_OK / _EMPTY / _TOO_LONG / _NO_MEMORY / _OVER_MAX */
    uint32_t *score;  /* == AlignmentResult.Score of the same pair; 0 unless status is OK */
} wfahip_scores;
int  wfahip_score_batch(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *seq_blob, uint64_t blob_bytes,
                        const uint64_t *q_off, const uint32_t *q_len, const uint64_t *t_off, const uint32_t *t_len,
                        uint64_t n_pairs, uint32_t max_score, wfahip_scores *out);
void wfahip_scores_free(wfahip_scores *s);

/* Score matrix: every query against every target, score only.  Query i is seq_blob[q_off[i] .. +q_len[i]), target j is
 * seq_blob[t_off[j] .. +t_len[j]); queries and targets may share sequences or be the same arrays (all against all).  Cell (i, j)
 * is written to status[i * out_stride + j] and score[i * out_stride + j] (out_stride 0 = n_t) and equals what wfahip_score_batch
 * returns for the pair (query i, target j) under the same p and max_score -- status, score and WFAHIP_PAIR_OVER_MAX alike, global
 * or semi-global, with wf-adaptive on or off, any penalties, any bytes.  The full rectangle is computed: under wf-adaptive
 * score(q, t) need not equal score(t, q).  Elements outside the n_q x n_t window of a strided output are never written, so a
 * caller may fill one tile of a larger matrix per call (or per GPU).  The outputs are the caller's; nothing is allocated that
 * the caller must free.  Whole-call errors, checked before any device work: WFAHIP_ERR_BAD_ARG for a null ctx, p, status or
 * score, a null offset or length array whose count is non-zero, a non-empty sequence within WFAHIP_MAX_SEQ_LEN that lies
 * outside the blob, 0 < out_stride < n_t, or (n_q - 1) * stride + n_t beyond 64 bits; then the params as wfahip_align_batch
 * checks them.  n_q == 0 or n_t == 0 returns WFAHIP_OK and touches nothing.
 * Each of the n_q + n_t sequences is 2-bit packed and checked once, and uploaded once (a quarter of its bytes); the cells run in
 * rectangular tiles on the matrix instances of the score kernels, global alignments on wfa_score_kernel, semi-global ones on
 * wfa_wide_kernel, each cell staging its two sequences from that table.  A tile's results download while the next tile runs.
 * Global cells with a sequence longer than 2 047 bases run on wfa_score_long_kernel<MATRIX>, a second launch over the same tile
 * that reads the table's words through sliding windows, when the matrix holds at least 64 such cells (DEBUG option
 * "score_long_min"); fewer take the full path.
 * The cells the score kernels cannot take -- a sequence with a byte outside ACGT, a semi-global sequence longer than 2 047 bases, a
 * band wider than the kernels' 248 diagonals, every cell of a penalty shape without an instance -- are aligned by the full path of
 * wfahip_align_batch in batches of bounded size, and only their score kept.  wfahip_last_timing: main_kernel_kind 21 (global; 24
 * when wfa_score_long_kernel took more cells than wfa_score_kernel) or 22 (semi-global) unless every cell took the full path,
 * n_retried_pairs = cells that took the full path (saturating at UINT32_MAX), arena_bytes = 0 unless some did. */
int  wfahip_score_matrix(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *seq_blob, uint64_t blob_bytes,
                         const uint64_t *q_off, const uint32_t *q_len, uint64_t n_q,
                         const uint64_t *t_off, const uint32_t *t_len, uint64_t n_t,
                         uint32_t max_score, int32_t *status, uint32_t *score, uint64_t out_stride);
/* ... with a flag per query ROW (q_rc: n_q flags, NULL = none set): every cell of a flagged row scores the reverse complement of its
 * query, and equals what wfahip_score_batch returns for the bytes (revcomp(query i), target j); the other rows, and every call with
 * q_rc = NULL, are wfahip_score_matrix, which is this entry without flags.  The complement of a byte: A <-> T, C <-> G, a <-> t,
 * c <-> g, every other byte itself.  The table still holds each sequence once, forward (with the same arrays on both sides a flagged
 * query is still a forward target): the kernels reverse-complement a flagged row's words as they stage them.  A flagged query with a
 * byte outside ACGT takes the full path like any such cell, on bytes reverse-complemented on the host. */
int  wfahip_score_matrix_rc(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *seq_blob, uint64_t blob_bytes,
                            const uint64_t *q_off, const uint32_t *q_len, uint64_t n_q, const uint8_t *q_rc,
                            const uint64_t *t_off, const uint32_t *t_len, uint64_t n_t,
                            uint32_t max_score, int32_t *status, uint32_t *score, uint64_t out_stride);

/* Device-resident variant: every pointer is a device address on the context's GPU (caller-owned).
 * d_rec receives n_pairs records of WFAHIP_REC_WORDS u32; d_ops receives the CIGAR ops
 * (capacity ops_cap entries; record fields OPS_OFF/OPS_LEN index into it).  max_len = an upper
 * bound of every q_len/t_len (0 = let the library compute it).  stream = hipStream_t to launch on
 * (NULL = the context's own stream).  Synchronous: returns when results are complete.
 * If ops_cap is too small the call returns WFAHIP_ERR_OOM and *ops_needed (if non-NULL) holds
 * the required capacity.
 * Memory behind a sequence: the packing pass reads a sequence that starts at a 16-byte boundary in 16-byte pieces, its last
 * piece too.  The allocation behind d_seq_blob must therefore be readable up to the next 16-byte boundary behind the last
 * base of every sequence (every device allocator's granularity gives that; a view that ends inside a larger allocation has it
 * as well).  The bytes read there do not influence any result.  This holds for every device entry that takes d_seq_blob
 * (wfahip_align_batch_bounded_device, wfahip_pack_pairs_device, wfahip_debug_prepack).
 * Memory behind packed words: the entry that takes device-resident words (wfahip_align_batch_packed_device) needs d_packed
 * readable for 16 bytes behind its n_words words; those bytes do not influence any result either. */
int  wfahip_align_batch_device(wfahip_ctx *ctx, const wfahip_params *p, const void *d_seq_blob,
                               uint64_t blob_bytes, const void *d_q_off, const void *d_q_len,
                               const void *d_t_off, const void *d_t_len, uint64_t n_pairs,
                               uint32_t max_len, void *d_rec, void *d_ops, uint64_t ops_cap,
                               uint64_t *ops_needed, void *stream);

/* Full alignment under a score bound: CIGARs for the pairs that pass a threshold, an early stop for the others.  Arguments,
 * ownership and whole-call errors are those of wfahip_align_batch / wfahip_align_batch_device.
 *   max_score == 0    no bound: the result equals the unbounded entry's in every field.
 *   score <= max_score  a pair the unbounded entry reports as WFAHIP_PAIR_OK with such a score comes back identical, every field
 *                     and every CIGAR op.
 *   score > max_score   status WFAHIP_PAIR_OVER_MAX, every other field 0, ops_len and ops_off 0 (device: the record is {8, 0, .., 0}).
 * WFAHIP_PAIR_EMPTY and _TOO_LONG are unchanged.  A pair the unbounded entry reports as WFAHIP_PAIR_NO_MEMORY may come back
 * WFAHIP_PAIR_OVER_MAX (it stops earlier), never the reverse.  For every pair, status and score equal what
 * wfahip_score_batch(.., max_score) returns -- the exact definition of "over" given there -- global or semi-global, wf-adaptive
 * on or off, any penalties, any bytes.
 * Where the bound STOPS a pair: the sub-wave forward kernels with row-indexed arenas (main_kernel_kind 3..6, 8..15) get arena
 * slots of max_score / g + 1 rows (g = gcd of the penalties) instead of rows for half the read length -- a pair that runs out
 * of them is over and final, it visits no retry rung and grows no arena; and wfa_generic_kernel ends a global pair when its
 * score step passes the bound.  Where it only FILTERS, after the alignment is done: semi-global pairs, the team kernels, the
 * two first-generation sub-wave kernels (kinds 1, 2).
 * Host entry: out->ops is dense in pair order, as from wfahip_align_batch.  Device entry: d_ops may hold unreferenced ops of
 * pairs that were filtered after their backtrace, and *ops_needed counts them.  wfahip_last_timing as after the unbounded
 * entries; pairs finalised as over by a pass do not count in n_retried_pairs. */
int  wfahip_align_batch_bounded(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *seq_blob,
                                uint64_t blob_bytes, const uint64_t *q_off, const uint32_t *q_len,
                                const uint64_t *t_off, const uint32_t *t_len, uint64_t n_pairs,
                                uint32_t max_score, wfahip_results *out);
int  wfahip_align_batch_bounded_device(wfahip_ctx *ctx, const wfahip_params *p, const void *d_seq_blob,
                                       uint64_t blob_bytes, const void *d_q_off, const void *d_q_len,
                                       const void *d_t_off, const void *d_t_len, uint64_t n_pairs,
                                       uint32_t max_len, uint32_t max_score, void *d_rec, void *d_ops, uint64_t ops_cap,
                                       uint64_t *ops_needed, void *stream);

/* Score only on device-resident input: wfahip_score_batch for a batch that already lives in HBM -- the output of
 * wfahip_generate_pairs_device, a torch pipeline, the candidates of an earlier GPU stage -- with the results left there for the next
 * stage.  Conventions as wfahip_align_batch_device: every pointer is a device address on the context's GPU and stays the caller's;
 * d_q_off / d_t_off are u64, d_q_len / d_t_len u32; max_len = an upper bound of every length (0 = the library finds it, on the
 * device); stream = hipStream_t to launch on (NULL = the context's own).  Synchronous: returns when the results are complete.
 * d_status (int32) and d_score (uint32) receive n_pairs elements each and nothing beyond them; the inputs are never written.
 * For every pair, d_status[i] and d_score[i] equal what wfahip_score_batch returns for the same bytes, params and max_score
 * (WFAHIP_PAIR_OK / _EMPTY / _TOO_LONG / _NO_MEMORY / _OVER_MAX, score 0 unless OK), and the same kernels do the work.
 * Whole-call errors: WFAHIP_ERR_BAD_ARG for a null ctx or p, or with n_pairs > 0 a null offset, length or output pointer (or a null
 * blob with blob_bytes > 0) -- checked before the device is touched; then the params as wfahip_align_batch checks them; n_pairs == 0
 * returns WFAHIP_OK and touches nothing.  The offsets cannot be seen from the host: wfa_score_plan_kernel checks, from the offset and
 * length arrays alone, that every non-empty pair within WFAHIP_MAX_SEQ_LEN lies inside [0, blob_bytes), and a batch that fails
 * returns WFAHIP_ERR_BAD_ARG with the outputs untouched BEFORE any kernel that reads a sequence byte is launched.
 * What the host entry does with the sequences in its hands happens on the device (wfa_score_dev.hpp): the long global pairs are
 * listed by a scan in batch order and 2-bit packed from the caller's blob by wfa_score_pack_kernel; the pairs the score kernels hand
 * back are gathered in pair order by wfa_score_redo_kernel (their offsets keep pointing into the caller's blob) and aligned by the
 * full path of wfahip_align_batch_device into buffers of the context; wfa_score_finish_kernel writes d_status / d_score.  Apart from
 * the kernel arguments, three fetches of 64 bytes of counters per call cross PCIe, plus what the full path itself fetches when
 * pairs take it.  wfahip_last_timing as after wfahip_score_batch (main_kernel_kind 19 / 23 / 20, n_retried_pairs, arena_bytes). */
int  wfahip_score_batch_device(wfahip_ctx *ctx, const wfahip_params *p, const void *d_seq_blob, uint64_t blob_bytes,
                               const void *d_q_off, const void *d_q_len, const void *d_t_off, const void *d_t_len,
                               uint64_t n_pairs, uint32_t max_len, uint32_t max_score, void *d_status, void *d_score,
                               void *stream);

/* Pre-packed input: the sequences arrive 2-bit packed, 16 bases per uint32 (base i of a
 * sequence in bits 2(i%16).. of word i/16, code = (ascii >> 1) & 3: A 0, C 1, T 2, G 3), every sequence starting at a
 * word boundary and followed by one pad word; pair i is packed[q_woff[i] ..] (q_len[i] bases) vs packed[t_woff[i] ..].
 * A quarter of the bytes cross PCIe, and they stay words on the device: a pass that fetches pre-packed pairs -- the first
 * pass of a large batch of 240+ base reads, the long-read instances -- has its fixed-stride slots {n, m, status, -, q words,
 * t words} copied from the uploaded words (wfa_prepack_words_kernel), and a pass that reads bytes (the retry rungs, the
 * lane-per-pair kernel, the long-pair kernels) has exactly its pairs expanded first (wfa_unpack_pairs_kernel: a thousandth
 * of a 1e6 x 1 kbp batch).  Rounds 2-3 expanded everything to bytes and packed it again (option "unpack_all" = 1).  Valid
 * only for pure uppercase ACGT input -- the reference compares raw bytes (wfa.go:408-454), so anything else must use
 * wfahip_align_batch.  wfahip_pack_pairs is the host-side packer (n_threads host threads; returns
 * WFAHIP_ERR_UNSUPPORTED if a byte outside ACGT is found); packed must hold the sum over all sequences of
 * wfahip_packed_words(len) words.  Results are identical to wfahip_align_batch on the unpacked bytes.
 * Semi-global batches take wfa_wide_kernel as the byte entry's do (its instances with a packed prologue copy a pair's words
 * into LDS: no bytes in between); the pairs it hands on are expanded for the ladder like any other pass's. */
uint64_t wfahip_packed_words(uint32_t len);
int  wfahip_pack_pairs(const uint8_t *seq_blob, const uint64_t *q_off, const uint32_t *q_len, const uint64_t *t_off,
                       const uint32_t *t_len, uint64_t n_pairs, int n_threads, uint32_t *packed, uint64_t *q_woff,
                       uint64_t *t_woff, uint64_t *n_words);
int  wfahip_align_batch_packed(wfahip_ctx *ctx, const wfahip_params *p, const uint32_t *packed, uint64_t n_words,
                               const uint64_t *q_woff, const uint32_t *q_len, const uint64_t *t_woff,
                               const uint32_t *t_len, uint64_t n_pairs, wfahip_results *out);

/* Score only on pre-packed input: wfahip_score_batch over the words of wfahip_pack_pairs, so that a caller packs once, scores as
 * often as needed and aligns the survivors (wfahip_align_batch_packed with a subset of the same offsets) on ONE buffer.  Layout as
 * above: 16 bases per word, code (ascii >> 1) & 3, every sequence at a word boundary and followed by one pad word; pair i is
 * packed[q_woff[i] ..] (q_len[i] bases) against packed[t_woff[i] ..].  Valid only for what was pure uppercase ACGT.
 * The offsets may come in any order and may REPEAT: one packed query may face fifty packed targets without being stored fifty
 * times, and a target may be the query of another pair.  The bits of a sequence's last word beyond its last base, and its pad
 * word, may hold anything: no result depends on them.
 * For every pair, status and score equal what wfahip_score_batch returns for the unpacked bytes under the same p and max_score
 * (WFAHIP_PAIR_OK / _EMPTY / _TOO_LONG / _NO_MEMORY / _OVER_MAX, score 0 unless OK), global or semi-global, wf-adaptive on or off,
 * any penalties.  Release out with wfahip_scores_free.
 * Whole-call errors, checked before the device is touched: WFAHIP_ERR_BAD_ARG for a null ctx, p or out, for packed null with
 * n_words > 0, with n_pairs > 0 for a null offset or length array, and for a pair, neither empty nor over WFAHIP_MAX_SEQ_LEN, one
 * of whose sequences has woff + wfahip_packed_words(len) > n_words (an empty or too long pair's offsets are never looked at); then
 * the params as wfahip_align_batch checks them.  n_pairs == 0 returns WFAHIP_OK with a zeroed out.
 * The n_words words cross PCIe once, a quarter of the bytes, and the four arrays behind them; nothing else of the batch does.  The
 * same kernels do the work, in instances whose prologue copies a pair's words into LDS where the byte instances load and pack
 * bytes; wfa_score_long_kernel reads the long global pairs where they lie in the uploaded words (its table is built from the
 * offsets: no sequence is packed or uploaded twice).  The pairs the kernels hand back -- a band over 248 diagonals, a semi-global
 * read over 2 047 bases, a penalty shape without an instance, fewer than "score_long_min" long pairs -- have their words, and only
 * theirs, gathered into a buffer of the entry's own and go through the full path of wfahip_align_batch_packed under the bound.
 * wfahip_last_timing as after wfahip_score_batch (main_kernel_kind 19 / 23 / 20, n_retried_pairs = pairs that took the full path,
 * arena_bytes = 0 unless some did). */
int  wfahip_score_batch_packed(wfahip_ctx *ctx, const wfahip_params *p, const uint32_t *packed, uint64_t n_words,
                               const uint64_t *q_woff, const uint32_t *q_len, const uint64_t *t_woff, const uint32_t *t_len,
                               uint64_t n_pairs, uint32_t max_score, wfahip_scores *out);

/* The reverse strand of packed queries.  A read's orientation is unknown when a set is screened: the query and its reverse complement
 * are both candidates.  In the packed code the complement of a base is code ^ 2, so the kernels make a query's reverse complement from
 * the words they copy into LDS anyway -- nothing is reverse-complemented on the host, packed twice or uploaded twice.
 * q_rc: n_pairs flags (NULL = none set).  q_rc[i] != 0: pair i scores the reverse complement of its query against its target; its
 * status and score equal what wfahip_score_batch returns for the bytes (revcomp(query), target) under the same p and max_score.  A
 * pair whose flag is clear is a pair of wfahip_score_batch_packed, which IS this entry with q_rc = NULL: everything said there holds,
 * errors, empty and too long pairs (whose offsets are never looked at, whatever their flag) and timing included.  Offsets may
 * repeat, so both strands of a pair are the pair listed twice, once flagged.
 * Flagged global pairs of reads beyond 2 047 bases: wfa_rc_words_kernel writes their queries' reverse complements once, behind the
 * uploaded words on the device, and wfa_score_long_kernel reads them there -- once per distinct {offset, length}, however many
 * targets such a query is listed against: device memory of a quarter of a byte per base of those queries, nothing on the host or
 * the bus.  Flagged pairs the kernels hand back are gathered with the same word function on the host. */
int  wfahip_score_batch_packed_rc(wfahip_ctx *ctx, const wfahip_params *p, const uint32_t *packed, uint64_t n_words,
                                  const uint64_t *q_woff, const uint32_t *q_len, const uint64_t *t_woff, const uint32_t *t_len,
                                  const uint8_t *q_rc, uint64_t n_pairs, uint32_t max_score, wfahip_scores *out);
/* Host only, no device: dst[0 .. wfahip_packed_words(len)) = the reverse complement of the len bases packed at src, as
 * wfahip_pack_pairs would write it (the bits of the last word beyond the last base and the pad word zero) -- for the reverse-strand
 * survivors a caller hands to wfahip_align_batch_packed.  Reads src[0 .. (len + 15) / 16) only: the pad word and the bits beyond
 * the last base may hold anything.  src and dst must not overlap.  WFAHIP_ERR_BAD_ARG: dst null, src null with len > 0, len over
 * WFAHIP_MAX_SEQ_LEN. */
int  wfahip_revcomp_packed(const uint32_t *src, uint32_t len, uint32_t *dst);

/* Full alignment of the reverse strand of packed queries: the last step of pack once, score both strands, align the survivors -- with a
 * subset of the same offsets AND flags, on the same buffer.  Nothing is reverse-complemented on the host and nothing is uploaded twice.
 * q_rc: n_pairs flags (NULL = none set).  q_rc[i] != 0: every field of pair i and every CIGAR op equals what wfahip_align_batch returns
 * for the bytes (revcomp(query i), target i) under the same p; qbegin / qend are coordinates on the reverse-complemented query.  A pair
 * whose flag is clear is a pair of wfahip_align_batch_packed, which IS this entry with q_rc = NULL: results, whole-call errors (checked
 * before the device is touched), empty and too long pairs (whose offsets are never looked at, whatever their flag) and
 * wfahip_last_timing included.  Offsets may come in any order, may repeat, and may name one offset under different lengths and flags:
 * both strands of a pair are the pair listed twice, once flagged, and a query offset may point into the middle of a longer sequence.
 * Where the reverse complement is made: the passes that take words make it from the words (wfa_prepack_words_kernel for the slots of
 * the duo, lane and long-window first passes, the packed prologue of wfa_wide_kernel; wfa_rc.hpp has the word function); the passes
 * that read bytes -- the retry rungs, the lane kernel when it packs itself, the generic, team and long-pair kernels -- read a flagged
 * query at an address of its own in a MIRROR of the byte blob, which exists only in device memory and only in a call with a flag set:
 * byte 2 B + 47 - a is the complement of byte a of the B = 16 n_words bytes the words stand for, so the reverse complement of any
 * (offset, length) is a contiguous run of it, and wfa_unpack_pairs_kernel expands a flagged query word by word into it.  A call
 * with a flag set holds 2 B + 96 bytes of blob on the device in place of B + 32. */
int  wfahip_align_batch_packed_rc(wfahip_ctx *ctx, const wfahip_params *p, const uint32_t *packed, uint64_t n_words,
                                  const uint64_t *q_woff, const uint32_t *q_len, const uint64_t *t_woff, const uint32_t *t_len,
                                  const uint8_t *q_rc, uint64_t n_pairs, wfahip_results *out);

/* The packed entries on device-resident input: bytes in HBM -> words -> both strands aligned -> CIGAR text (wfahip_cigar_text_device)
 * without a sequence byte crossing PCIe.  Conventions as the other device entries: every pointer is a device address on the context's
 * GPU and stays the caller's; offsets are u64 and lengths u32; stream = hipStream_t to launch on (NULL = the context's own);
 * synchronous; the inputs are never written.
 *
 * wfahip_pack_pairs_device: wfahip_pack_pairs as kernels (wfa_amd/csrc/wfa_packdev.hip; the 16-bytes-to-a-word rule is
 * wfa_packdev.hpp's).  d_packed, d_q_woff[i] / d_t_woff[i] (u64) and *n_words receive exactly what the host packer writes for the
 * same bytes: the sequences follow one another as q0, t0, q1, t1, .., each at a word boundary and wfahip_packed_words(len) words
 * long; a length over WFAHIP_MAX_SEQ_LEN counts as 0 and gives one zero word; the bits of a sequence's last word beyond its last base
 * and its pad word are zero.  Each sequence is packed on its own: the query of a pair whose target is empty is packed.  No word at
 * or beyond the total is written.  wfahip_last_timing is not touched.
 *   WFAHIP_ERR_BAD_ARG before the context is dereferenced: a null ctx; with n_pairs > 0 a null offset, length or woff array; a
 *     null blob with blob_bytes > 0; a null d_packed with words_cap > 0; n_pairs beyond 0xFFFFFFF0.  n_pairs == 0 returns WFAHIP_OK
 *     with *n_words = 0 and touches nothing.
 *   WFAHIP_ERR_BAD_ARG with d_packed untouched, before any kernel that reads a sequence byte is launched: a sequence with
 *     0 < len <= WFAHIP_MAX_SEQ_LEN does not lie inside [0, blob_bytes) -- found on the device from the offset and length arrays
 *     alone, compared without a sum that could wrap.
 *   WFAHIP_ERR_OOM: words_cap is below the total; d_packed is untouched, the woff arrays are filled and *n_words holds the total --
 *     a caller sizes with d_packed = NULL, words_cap = 0 and calls again.
 *   WFAHIP_ERR_UNSUPPORTED: a byte INSIDE a packed sequence is outside uppercase ACGT (bytes before, between and behind the
 *     sequences do not count); the contents of d_packed are then undefined, the woff arrays valid.
 * Memory behind the blob as for wfahip_align_batch_device: readable up to the next 16-byte boundary behind every sequence; a
 * sequence whose address is not a multiple of 16 is read in aligned dwords.
 * Three passes: wfa_packdev_len_kernel (words per pair and the bounds check); an exclusive 64-bit scan in pair order, in place in
 * d_q_woff; wfa_packdev_pack_kernel, laid out over OUTPUT words -- a workgroup takes a tile of 1 024 words and finds its sequences
 * by a search in d_q_woff, a lane makes one word from 16 bytes --, so that 500 reads of 50 kbp and 1e6 reads of 100 bases both fill
 * the GPU.  Scratch lives in the context.  64 bytes of counters are fetched before the pack pass (the total, the bounds verdict) and
 * again behind it (the ACGT verdict); nothing else crosses PCIe.  WFAHIP_DEBUG_TIMING=1 prints the passes' times to stderr. */
int  wfahip_pack_pairs_device(wfahip_ctx *ctx, const void *d_seq_blob, uint64_t blob_bytes, const void *d_q_off,
                              const void *d_q_len, const void *d_t_off, const void *d_t_len, uint64_t n_pairs, void *d_packed,
                              uint64_t words_cap, void *d_q_woff, void *d_t_woff, uint64_t *n_words, void *stream);

/* wfahip_align_batch_packed_device: full alignment of device-resident words, both strands, optionally bounded.  d_rec, d_ops,
 * ops_cap, *ops_needed, max_len and WFAHIP_ERR_OOM on a short op buffer are those of wfahip_align_batch_device.  Every record field
 * and every op a record indexes equals what wfahip_align_batch_packed_rc returns for the same words, offsets, lengths and flags;
 * with max_score > 0 the result equals wfahip_align_batch_bounded's on the corresponding bytes (a pair over the bound: the record
 * {8, 0, .., 0}).  d_q_rc: a u8 per pair, NULL = none set; a call whose flags are all zero is the call without flags -- the same
 * route, no mirror.  Offsets may come in any order, repeat, and name one offset under different lengths and flags; the offsets of an
 * empty or too long pair are never looked at.
 * The caller's arrays are never written: the byte offsets the kernels take, and the mirror addresses of flagged queries, go into
 * scratch of the context, and so does the byte blob the byte-reading passes expand their pairs into (16 n_words + 32 bytes, 32
 * n_words + 96 with a flag set; nothing is expanded up front unless option "unpack_all" is 1).
 * Memory behind the words: d_packed must be readable for 16 bytes behind its n_words words (the slack the host entry gives its own
 * staging buffer); what is read there influences no result.
 *   WFAHIP_ERR_BAD_ARG before the context is dereferenced: a null ctx or p; with n_pairs > 0 a null offset, length or d_rec
 *     pointer; a null d_packed with n_words > 0; a null d_ops with ops_cap > 0.  Then the params as wfahip_align_batch checks them;
 *     n_pairs == 0 returns WFAHIP_OK.
 *   WFAHIP_ERR_BAD_ARG with d_rec and d_ops untouched, before any kernel that reads a packed word is launched: a pair, neither empty
 *     nor too long, has a sequence with woff + wfahip_packed_words(len) > n_words (compared without a sum that could wrap).
 * One kernel, wfa_packed_check_kernel, finds that on the device, and with it the longest read (max_len = 0), whether any flag is set,
 * and the scaled offsets; one 64-byte fetch brings its verdicts to the host.  wfahip_last_timing as after the host entry: for a
 * batch that entry does not slice (under 200 000 pairs), main_kernel_kind, n_packed_pairs and n_retried_pairs are the host entry's
 * on the same input when max_len is 0. */
int  wfahip_align_batch_packed_device(wfahip_ctx *ctx, const wfahip_params *p, const void *d_packed, uint64_t n_words,
                                      const void *d_q_woff, const void *d_q_len, const void *d_t_woff, const void *d_t_len,
                                      const void *d_q_rc, uint64_t n_pairs, uint32_t max_len, uint32_t max_score, void *d_rec,
                                      void *d_ops, uint64_t ops_cap, uint64_t *ops_needed, void *stream);

/* wfahip_score_batch_packed_device: the screen of the pipeline on device-resident words -- wfahip_score_batch_packed_rc for words,
 * offsets, lengths and flags that live in HBM, the results left there.  With it the chain pack (wfahip_pack_pairs_device) -> score
 * both strands under a bound -> survivors (wfahip_select_pairs_device) -> align (wfahip_align_batch_packed_device) -> text
 * (wfahip_cigar_text_device) runs with only counters crossing the bus.
 * Inputs as wfahip_align_batch_packed_device's: device pointers that stay the caller's and are never written; u64 word offsets, u32
 * lengths; d_q_rc a u8 per pair, NULL = none set; d_packed readable for 16 bytes behind its n_words words; max_len = 0 lets the
 * library find the longest read; stream = NULL is the context's own; synchronous.  Outputs as wfahip_score_batch_device's: d_status
 * (int32) and d_score (uint32) receive exactly n_pairs elements each and nothing beyond.
 * For every pair, status and score equal what wfahip_score_batch_packed_rc returns for the same words, offsets, lengths, flags,
 * params and max_score -- wfahip_score_batch on the bytes (revcomp(query) if flagged else query, target) -- and everything that entry
 * promises holds: offsets in any order, repeated, naming a prefix of a longer sequence; anything in the bits of a last word beyond
 * the last base and in the pad word; the offsets of an empty or too long pair never looked at, whatever its flag; a call whose flags
 * are all zero takes the route of the call with d_q_rc = NULL.
 *   WFAHIP_ERR_BAD_ARG before the context is dereferenced: a null ctx or p; with n_pairs > 0 a null offset, length or output pointer;
 *     a null d_packed with n_words > 0; n_pairs beyond 0xFFFFFFF0; n_words beyond 2^58.  Then the params as wfahip_align_batch checks
 *     them; n_pairs == 0 returns WFAHIP_OK and touches nothing.
 *   WFAHIP_ERR_BAD_ARG with the outputs untouched, before any kernel that reads a packed word is launched: a pair, neither empty nor
 *     too long, has a sequence with woff + wfahip_packed_words(len) > n_words (compared without a sum that could wrap).
 * The router is wfahip_score_batch_device's, on words (wfa_amd/csrc/wfa_score_dev.hpp): wfa_score_pkplan_kernel finds the bounds
 * verdict, the longest read, whether a flag is set and the long global pairs, and -- when there are at least "score_long_min" of them
 * -- writes wfa_score_long_kernel's table in batch order with offsets pointing INTO the caller's words; the packed pair-list
 * instances of the score kernels read the caller's arrays as they are.  A flagged long query is reverse-complemented into scratch of
 * the context by wfa_score_rcq_kernel and read from there.  Unlike the host entry there is no dedup by {offset, length}: one reverse
 * complement per flagged long pair, device memory of a quarter of a byte per base of every flagged long pair.  The pairs the kernels
 * hand back are listed in pair order, exactly their words are gathered into a buffer of the context (wfa_score_gather_kernel: a
 * flagged query through the same word function, tail bits and pad words cleared) and aligned by the full path of
 * wfahip_align_batch_packed_device under the bound, in chunks.  Apart from the kernel arguments, two fetches of 64 bytes of counters
 * per call cross PCIe, plus what the full path itself fetches when pairs take it.
 * wfahip_last_timing: main_kernel_kind (19 / 23 / 20) and n_retried_pairs are wfahip_score_batch_packed_rc's on the same input, and
 * arena_bytes is 0 exactly when that entry's is. */
int  wfahip_score_batch_packed_device(wfahip_ctx *ctx, const wfahip_params *p, const void *d_packed, uint64_t n_words,
                                      const void *d_q_woff, const void *d_q_len, const void *d_t_woff, const void *d_t_len,
                                      const void *d_q_rc, uint64_t n_pairs, uint32_t max_len, uint32_t max_score,
                                      void *d_status, void *d_score, void *stream);

/* wfahip_select_pairs_device: the survivors of a screen as the next stage's arrays -- a stable compaction, in pair order, of the
 * pairs with d_status[i] == WFAHIP_PAIR_OK (under a max_score the score entries have turned the others into WFAHIP_PAIR_OVER_MAX).
 * Every pointer but n_selected is a device address on the context's GPU and stays the caller's; the inputs are never written.
 * d_idx (u32, may be NULL) receives the selected indices; d_q_off_out / d_q_len_out / d_t_off_out / d_t_len_out / d_q_rc_out
 * (u64 / u32 / u64 / u32 / u8) the selected elements of the five input arrays.  Each has capacity n_pairs; only the first
 * *n_selected elements are written.  d_q_rc and d_q_rc_out are both NULL or both non-NULL.  The offsets are opaque u64 -- word
 * offsets and byte offsets both work --, so the output feeds wfahip_align_batch_packed_device or wfahip_align_batch_device unchanged.
 *   WFAHIP_ERR_BAD_ARG before the context is dereferenced: a null ctx or n_selected; with n_pairs > 0 a null d_status, input or _out
 *     array; d_q_rc without d_q_rc_out or the reverse; n_pairs beyond 0xFFFFFFF0.  n_pairs == 0 returns WFAHIP_OK with
 *     *n_selected = 0 and touches nothing else.
 * Two launches of wfa_score_select_kernel with the scan of wfahip_score_batch_device's router between them; scratch lives in the
 * context; one fetch of 64 bytes brings the count.  stream = hipStream_t (NULL = the context's own).  Synchronous.
 * wfahip_last_timing is not touched. */
int  wfahip_select_pairs_device(wfahip_ctx *ctx, const void *d_status, uint64_t n_pairs,
                                const void *d_q_off, const void *d_q_len, const void *d_t_off, const void *d_t_len, const void *d_q_rc,
                                void *d_idx, void *d_q_off_out, void *d_q_len_out, void *d_t_off_out, void *d_t_len_out, void *d_q_rc_out,
                                uint64_t *n_selected, void *stream);

/* CIGAR text, rendered where the ops are.  AlignmentResult.CIGAR(onlyAlignedRegion) (wfa_cigar.go:217-255) of every pair of a
 * batch as bytes: what a SAM / PAF writer puts into a file.  The rule (wfa_amd/csrc/wfa_cigar.hpp, one source for the kernels and
 * the host renderer): every op renders as the decimal of op & 0xFFFFFFFF -- a full u32, one to ten digits, no leading zero, a
 * count of 0 as "0" -- followed by the byte op >> 32, verbatim, whatever byte it is; the ops render in the order the record indexes
 * them.  only_aligned != 0 renders the ops from the first 'M' op to the last 'M' op, inclusive (trimOps); a pair without an 'M' op
 * (A against C, global: 1X), where the reference would panic, renders the empty string.  A pair's op count is OPS_LEN when its
 * status is WFAHIP_PAIR_OK, else 0 -- the records of failed pairs may hold stale words: empty, too long, no-memory and over-max
 * pairs render the empty string.
 *
 * wfahip_cigar_text_device: d_rec / d_ops as wfahip_align_batch_device (or _bounded_device) left them, or any records and ops of
 * that layout; every pointer is a device address on the context's GPU and stays the caller's.  Pair i's text is
 * d_text[d_text_off[i] .. d_text_off[i + 1]), without terminators; d_text_off (u64[n_pairs + 1], 8-byte aligned) starts at 0 and
 * ends at the total, which *text_needed (if non-NULL) receives.  No byte of d_text at or beyond the total is written; d_rec and
 * d_ops are never written.  text_cap below the total: WFAHIP_ERR_OOM with d_text untouched and d_text_off filled -- a caller sizes
 * with d_text = NULL, text_cap = 0 and calls again.  An OK pair whose ops leave [0, ops_cap) (OPS_LEN > ops_cap or OPS_OFF >
 * ops_cap - OPS_LEN): WFAHIP_ERR_BAD_ARG with d_text untouched, before the kernel that reads those ops to write text is launched
 * (d_text_off then holds nothing of use).  WFAHIP_ERR_BAD_ARG before the context is dereferenced: a null ctx; with n_pairs > 0 a
 * null d_rec or d_text_off; a null d_ops with ops_cap > 0; a null d_text with text_cap > 0; n_pairs beyond 0xFFFFFFF0.
 * n_pairs == 0 returns WFAHIP_OK with *text_needed = 0 and writes d_text_off[0] = 0 when d_text_off is non-null (the only case in
 * which it touches the context or the device).  stream = hipStream_t (NULL = the context's own).  Synchronous.  wfahip_last_timing
 * is not touched.
 * Three passes (wfa_cigar.hip): wfa_cigar_len_kernel, a wave per pair -- the trimmed range from ballots, the text length from
 * compares; an exclusive 64-bit scan of the lengths in pair order, in place in d_text_off; wfa_cigar_write_kernel, a wave per pair
 * in rounds of 64 ops, each lane rendering its op where a wave prefix sum puts it.  Scratch lives in the context and is allocated
 * once per shape; one fetch of 64 bytes of counters per call crosses PCIe.  1e6 x 1 kbp pairs, 92 ops each: 0.96 ms for the three
 * passes (136 ms for wfahip_cigar_text on 16 host threads).  WFAHIP_DEBUG_TIMING=1 prints the passes' times to stderr. */
int  wfahip_cigar_text_device(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap,
                              uint64_t n_pairs, int only_aligned, void *d_text, uint64_t text_cap,
                              void *d_text_off /* u64[n_pairs + 1] */, uint64_t *text_needed, void *stream);

/* Host only, no device, no context: the same bytes for a wfahip_results in host memory (n_threads host threads over contiguous
 * ranges of pairs, the same header functions as the kernels).  out->text holds n_bytes bytes (NULL when n_bytes == 0), out->off
 * n + 1 offsets, off[0] = 0 and off[n] = n_bytes; both are malloc'd and released with wfahip_cigars_free.  r->n == 0 gives
 * n = n_bytes = 0, text = NULL and off pointing at one 0.  WFAHIP_ERR_BAD_ARG (out zeroed, when there is one): a null r or out;
 * with r->n > 0 a null status, ops_off or ops_len; a null ops with n_ops > 0; an OK pair with ops_off[i] + ops_len[i] > n_ops. */
typedef struct { uint64_t n; uint64_t n_bytes; char *text; uint64_t *off; /* n + 1 */ } wfahip_cigars;
int  wfahip_cigar_text(const wfahip_results *r, int only_aligned, int n_threads, wfahip_cigars *out);
void wfahip_cigars_free(wfahip_cigars *c);

/* Host blobs in, fields + CIGAR text out: no ops cross PCIe.  Inputs and whole-call errors as wfahip_align_batch, checked first
 * (plus WFAHIP_ERR_BAD_ARG for a null cig).  out has every field array of wfahip_align_batch for the same input; ops_len is the
 * op count, ops_off is all 0, ops == NULL and n_ops == 0 (release with wfahip_results_free, as ever).  cig holds the text of
 * wfahip_cigar_text(.., only_aligned) over that entry's results, byte for byte (release with wfahip_cigars_free).
 * The PLAIN path only: one upload of the blob and the four arrays, the alignment with its op-capacity retry, the three kernels
 * above, one download of records, text and offsets, the records unpacked on the host.  There is no slicing, no overlap of the
 * upload with the alignment and no autopack -- what wfahip_align_batch does for batches of 200 000 pairs and more.  Measured on
 * 1e6 x 1 kbp pairs it is the faster way to the text all the same (160 ms host to host against 224 ms for wfahip_align_batch
 * followed by wfahip_cigar_text on 16 threads: 215 MB of text leave the device in place of 737 MB of ops; KERNELS.md 4p).  A
 * caller picks by what it needs: this entry where the text is the product and the ops are not. */
int  wfahip_align_batch_text(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *seq_blob, uint64_t blob_bytes,
                             const uint64_t *q_off, const uint32_t *q_len, const uint64_t *t_off, const uint32_t *t_len,
                             uint64_t n_pairs, int only_aligned, wfahip_results *out, wfahip_cigars *cig);

/* The display rows, rendered where the ops and the sequences are.  AlignmentResult.AlignmentText(q, t, onlyAlignedRegion)
 * (wfa_cigar.go:259-333) of every pair of a batch: a query row, a row of bars and a target row of one length, one column per
 * aligned or gapped base.  The rule (wfa_amd/csrc/wfa_altext.hpp, one source for the kernels and the host renderer): the count
 * columns of an op are, in the three rows, M: query byte, '|', target byte; X: query byte, ' ', target byte; I: '-', ' ', target
 * byte; D and H: query byte, ' ', '-'.  An op of any other letter has no column and consumes nothing, a count of 0 gives no
 * column, and sequence bytes are copied verbatim, whatever they are.  only_aligned == 0 renders all ops over the whole sequences.
 * only_aligned != 0 renders the ops from the first 'M' op to the last (as the CIGAR text does) over the windows the RECORD names,
 * read as int32: query bytes [QBEGIN - 1, QEND) and target bytes [TBEGIN - 1, TEND); the bases of the trimmed-away ops are not
 * summed.  A pair's rows are empty when its status is not WFAHIP_PAIR_OK, when OPS_LEN is 0 and, under only_aligned, when it has
 * no 'M' op (where the reference would panic).
 * Where the reference would index out of range the call fails, checked for every OK pair with an op that renders: its ops lie in
 * [0, ops_cap) (the CIGAR entry's two compares); both sequences lie in [0, blob_bytes); trimmed, 1 <= BEGIN, BEGIN - 1 <= END and
 * END <= the sequence's length, for both; the query and the target bases its ops consume, as 64-bit sums, do not exceed the
 * window's length.  The library's results meet them with equality, with one exception that is the reference's own: under
 * wf-adaptive its ops now and then consume one base more than both sequences hold (pair 61 309 of the 1 kbp benchmark batch ends
 * ..5M1X3I over a query of 1 000 bases; the CPU oracle returns the same ops).  Untrimmed, a batch with such a pair is refused;
 * trimmed it renders, the windows being the record's.  A caller sets the pair aside: wfahip_check_alignments_device under the mask
 * WFAHIP_CHK_NO_ROWS names it (scripts/alignment_text_bench.py does that).
 *
 * wfahip_alignment_text_device: d_rec / d_ops as wfahip_align_batch_device (or _bounded_device) left them, or any records and ops
 * of that layout; the blob and the four arrays (offsets u64, lengths u32) are the ones that call was given.  Only bytes inside the
 * sequences are read: the blob needs NO readable bytes behind blob_bytes for this entry.  Every pointer is a device address on
 * the context's GPU and stays the caller's.  Pair i's rows are d_q_row, d_a_row and d_t_row[d_row_off[i] .. d_row_off[i + 1]):
 * three planes, one offset array (u64[n_pairs + 1], 8-byte aligned) that starts at 0 and ends at the total -- the bytes of ONE
 * plane -- which *row_needed (if non-NULL) receives.  No byte of a plane at or beyond the total is written; no input is written.
 * Planes that are all 4-byte aligned are written four columns to a store, others byte by byte.  row_cap (the capacity of each
 * plane) below the total: WFAHIP_ERR_OOM with the planes untouched and d_row_off filled -- a caller sizes with null planes and
 * row_cap = 0 and calls again.  A failed check of the paragraph above: WFAHIP_ERR_BAD_ARG with the planes untouched, before the
 * kernel that reads ops or sequence bytes to write rows is launched (d_row_off then holds nothing of use).  WFAHIP_ERR_BAD_ARG
 * before the context is dereferenced: a null ctx; with n_pairs > 0 a null d_rec, d_row_off, d_q_off, d_q_len, d_t_off or d_t_len;
 * a null d_ops with ops_cap > 0; a null d_seq_blob with blob_bytes > 0; a null plane with row_cap > 0; n_pairs beyond 0xFFFFFFF0.
 * n_pairs == 0 returns WFAHIP_OK with *row_needed = 0 and writes d_row_off[0] = 0 when d_row_off is non-null (the only case in
 * which it touches the context or the device).  stream = hipStream_t (NULL = the context's own).  Synchronous.  wfahip_last_timing
 * is not touched.
 * Three passes (wfa_cigar.hip): wfa_altext_len_kernel, a wave per pair -- the range from ballots, the columns and the bases as
 * three 64-bit sums, the checks; the CIGAR entry's scan, in place in d_row_off; wfa_altext_write_kernel, a wave per pair in rounds
 * of 64 ops, the round's starts in LDS, the lanes sweeping the round's columns four to a lane (KERNELS.md 4q).  Scratch lives in
 * the context; one fetch of 64 bytes of counters per call crosses PCIe.  1e6 x 1 kbp pairs, 3 x 1 014 bytes each: 4.5 ms for the
 * three passes (1.04 s for wfahip_alignment_text on 16 host threads).  WFAHIP_DEBUG_TIMING=1 prints the passes' times to stderr. */
int  wfahip_alignment_text_device(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap,
                                  const void *d_seq_blob, uint64_t blob_bytes, const void *d_q_off, const void *d_q_len,
                                  const void *d_t_off, const void *d_t_len, uint64_t n_pairs, int only_aligned,
                                  void *d_q_row, void *d_a_row, void *d_t_row, uint64_t row_cap,
                                  void *d_row_off /* u64[n_pairs + 1] */, uint64_t *row_needed, void *stream);

/* Host only, no device, no context: the same bytes and offsets for a wfahip_results in host memory and the blob and arrays it was
 * aligned from (n_threads host threads over contiguous ranges of pairs, the same header functions as the kernels).  The trimmed
 * windows are r->qbegin / qend / tbegin / tend.  out->q_row, a_row and t_row hold n_bytes bytes each (NULL when n_bytes == 0),
 * out->off n + 1 offsets, off[0] = 0 and off[n] = n_bytes; all are malloc'd and released with wfahip_align_texts_free.  r->n == 0
 * gives n = n_bytes = 0, null rows and off pointing at one 0.  WFAHIP_ERR_BAD_ARG (out zeroed, when there is one): a null r or
 * out; with r->n > 0 a null status, ops_off, ops_len, offset or length array, and under only_aligned a null qbegin, qend, tbegin
 * or tend; a null ops with n_ops > 0; a null seq_blob with blob_bytes > 0; a pair that fails a check of the device entry (with
 * n_ops as ops_cap). */
typedef struct { uint64_t n, n_bytes; char *q_row, *a_row, *t_row; uint64_t *off; /* n + 1 */ } wfahip_align_texts;
int  wfahip_alignment_text(const wfahip_results *r, const uint8_t *seq_blob, uint64_t blob_bytes, const uint64_t *q_off,
                           const uint32_t *q_len, const uint64_t *t_off, const uint32_t *t_len, int only_aligned,
                           int n_threads, wfahip_align_texts *out);
void wfahip_align_texts_free(wfahip_align_texts *t);

/* The display rows from 2-bit packed words, both strands: the last product of the chain pack (wfahip_pack_pairs_device) -> score ->
 * select -> align (wfahip_align_batch_packed_device) -> text, with no sequence byte anywhere.  For a flagged pair (q_rc[i] != 0) the
 * record's QBEGIN / QEND and every op are coordinates on the reverse-complemented query, bytes that exist nowhere a caller can point
 * to: the rows are rendered straight from the words, a flagged query reverse-complemented as it is read.  The decoding rule
 * (wfa_amd/csrc/wfa_altext_pk.hpp, one source for the kernels and the host renderer): the letter of a code is "ACTG"[code]; base p of
 * a forward sequence is bits 2 (p % 16) .. of word p / 16; base p of a flagged query of len bases is the complement (code ^ 2) of
 * forward base len - 1 - p.  The rows equal, byte for byte, what wfahip_alignment_text_device writes for the same records and ops
 * over a byte blob in which pair i's query is the letters of its words, reverse-complemented if flagged, and its target the letters
 * of its words.
 *
 * wfahip_alignment_text_packed_device: d_rec / d_ops as wfahip_align_batch_packed_device left them, or any records and ops of that
 * layout; the words, the offsets (u64), lengths (u32) and flags (u8 per pair, NULL = none set) are the ones that call was given.
 * Offsets may come in any order, repeat, and name one offset under different lengths and flags; the offsets of a pair that renders
 * nothing (status not OK, OPS_LEN 0, no column, no 'M' op under only_aligned) are never looked at.  Of a sequence that renders only
 * words in [woff, woff + wfahip_packed_words(len)) are read; no result depends on the bits of its last word beyond its last base or
 * on its pad word; d_packed needs NO readable memory behind its n_words words for this entry.
 * Planes, d_row_off, *row_needed, row_cap, WFAHIP_ERR_OOM (planes untouched, d_row_off filled: size with null planes and row_cap = 0,
 * call again), n_pairs == 0, stream, synchrony and wfahip_last_timing (untouched) are wfahip_alignment_text_device's, word for word;
 * no input is written.  The checks, made for every OK pair with an op that renders, are that entry's with the blob check replaced:
 * the ops lie in [0, ops_cap); for both sequences woff <= n_words and wfahip_packed_words(len) <= n_words - woff (compared without a
 * sum that could wrap); trimmed, 1 <= BEGIN, BEGIN - 1 <= END and END <= the sequence's length; the query and target bases the ops
 * consume, as 64-bit sums, do not exceed the window.  A failed check: WFAHIP_ERR_BAD_ARG with the planes untouched, before the kernel
 * that reads ops or words to write rows is launched.  The wf-adaptive pair whose ops consume one base more than the sequences hold
 * is refused untrimmed and renders trimmed, as there.  WFAHIP_ERR_BAD_ARG before the context is dereferenced: a null ctx; with
 * n_pairs > 0 a null d_rec, d_row_off, d_q_woff, d_q_len, d_t_woff or d_t_len; a null d_ops with ops_cap > 0; a null d_packed with
 * n_words > 0; a null plane with row_cap > 0; n_pairs beyond 0xFFFFFFF0.
 * Three passes (wfa_cigar.hip): wfa_altext_pk_len_kernel, the byte entry's length kernel with the window check on words; the same
 * scan; wfa_altext_pk_write_kernel, the byte entry's rounds, groups and stores, a group of four columns inside one op taking its
 * letters from two words by a funnel shift and one v_perm_b32, a flagged query's from the four bases that end at len - 1 - p
 * (KERNELS.md 4t).  1e6 x 1 kbp pairs, every second one flagged, 3 x 1 014 bytes each: 4.9 ms for the three passes against 4.3 ms for
 * wfahip_alignment_text_device on the same records over bytes -- the decoding costs 0.6 ms of the write pass.  WFAHIP_DEBUG_TIMING=1
 * prints the passes' times to stderr. */
int  wfahip_alignment_text_packed_device(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap,
                                         const void *d_packed, uint64_t n_words, const void *d_q_woff, const void *d_q_len,
                                         const void *d_t_woff, const void *d_t_len, const void *d_q_rc /* u8 per pair, NULL = none */,
                                         uint64_t n_pairs, int only_aligned, void *d_q_row, void *d_a_row, void *d_t_row,
                                         uint64_t row_cap, void *d_row_off /* u64[n_pairs + 1] */, uint64_t *row_needed, void *stream);

/* Host only, no device, no context: the same bytes and offsets for a wfahip_results in host memory -- wfahip_align_batch_packed_rc's,
 * or wfahip_align_batch_packed's with q_rc = NULL -- and the words, offsets, lengths and flags it was aligned from.  Everything else
 * as wfahip_alignment_text: the same out, released with wfahip_align_texts_free and zeroed on an error; n_threads host threads; the
 * same header functions as the kernels; WFAHIP_ERR_BAD_ARG for a null r or out, with r->n > 0 a null status, ops_off, ops_len,
 * offset or length array, under only_aligned a null qbegin, qend, tbegin or tend, a null ops with n_ops > 0, a null packed with
 * n_words > 0, and a pair that fails a check of the device entry (with n_ops as ops_cap). */
int  wfahip_alignment_text_packed(const wfahip_results *r, const uint32_t *packed, uint64_t n_words, const uint64_t *q_woff,
                                  const uint32_t *q_len, const uint64_t *t_woff, const uint32_t *t_len,
                                  const uint8_t *q_rc /* NULL = none */, int only_aligned, int n_threads, wfahip_align_texts *out);

/* The difference string, rendered where the ops and the sequences are: minimap2's cs tag (short form) of every pair of a batch, the
 * compact text product that names the bases.  The CIGAR text carries no base; the display rows carry every base three planes wide.
 * This string writes match runs as counts and spells out only what differs, so that from the TARGET -- the reference sequence of the
 * string -- and the string the aligned query is rebuilt exactly.  The rule (wfa_amd/csrc/wfa_diff.hpp, one source for the kernels and
 * the host renderers), per op word letter << 32 | count, in op order:
 *     M          ':' and the decimal of count (the CIGAR text's u32 decimal)       1 + digits bytes, reads no base
 *     X          per column '*', lc(target byte), lc(query byte)                   3 count bytes
 *     I          '-' and lc of the count target bytes (the target alone has them)  1 + count bytes
 *     D, H       '+' and lc of the count query bytes (the query alone has them)    1 + count bytes
 * An op of any other letter renders nothing and consumes nothing; an op of count 0 renders nothing.  Bases are consumed exactly as
 * the display rows consume them.  lc(b) is b + 32 for 'A' <= b <= 'Z'; every other byte is copied verbatim.  Ops are taken at face
 * value: an M op is never compared with the sequences (WFAHIP_CHK_M_DIFFERS of the check is how a caller sees the reference's rare
 * mismatching M column), and neighbouring ops of one letter are not merged -- library results never have them, synthetic input
 * renders one token per op.  Lengths are 64-bit sums: one X op may render 3 x 0xFFFFFFFF bytes.
 * Which ops render is wfahip_alignment_text_device's, exactly: only_aligned == 0 renders all ops over the whole sequences;
 * only_aligned != 0 the ops from the first 'M' op to the last over the windows the RECORD names, read as int32 -- query bytes
 * [QBEGIN - 1, QEND) and target bytes [TBEGIN - 1, TEND).  A pair renders the empty string when its status is not WFAHIP_PAIR_OK,
 * when OPS_LEN is 0, when trimmed it has no 'M' op, and when none of its ops renders a byte.  The checks are that entry's too, made
 * by the same functions in the same order for every OK pair with an op that renders: the ops lie in [0, ops_cap); both sequences lie
 * inside the blob; trimmed, 1 <= BEGIN, BEGIN - 1 <= END and END <= the sequence's length; the bases the ops consume, as 64-bit sums,
 * fit the windows.  A batch with the wf-adaptive pair whose ops consume one base more than the sequences hold is refused untrimmed
 * and renders trimmed, as there.
 *
 * wfahip_diff_text_device: d_rec / d_ops, the blob and the four arrays as wfahip_alignment_text_device takes them; only bytes inside
 * the sequences are read, and an M op reads none: the blob needs NO readable bytes behind blob_bytes.  Every pointer is a device
 * address on the context's GPU and stays the caller's.  Pair i's text is d_text[d_text_off[i] .. d_text_off[i + 1]), without
 * terminators; d_text_off (u64[n_pairs + 1], 8-byte aligned) starts at 0 and ends at the total, which *text_needed (if non-NULL)
 * receives.  No byte of d_text at or beyond the total is written; no input is written.  text_cap below the total: WFAHIP_ERR_OOM
 * with d_text untouched and d_text_off filled -- a caller sizes with d_text = NULL, text_cap = 0 and calls again.  A failed check of
 * the paragraph above: WFAHIP_ERR_BAD_ARG with d_text untouched, before the kernel that reads a sequence byte to write text is
 * launched (d_text_off then holds nothing of use).  WFAHIP_ERR_BAD_ARG before the context is dereferenced: a null ctx; with
 * n_pairs > 0 a null d_rec, d_text_off, d_q_off, d_q_len, d_t_off or d_t_len; a null d_ops with ops_cap > 0; a null d_seq_blob with
 * blob_bytes > 0; a null d_text with text_cap > 0; n_pairs beyond 0xFFFFFFF0.  n_pairs == 0 returns WFAHIP_OK with *text_needed = 0
 * and writes d_text_off[0] = 0 when d_text_off is non-null (the only case in which it touches the context or the device).  stream =
 * hipStream_t (NULL = the context's own).  Synchronous.  wfahip_last_timing is not touched.
 * Three passes (wfa_cigar.hip): wfa_diff_len_kernel, the display rows' length kernel with a fourth 64-bit sum, the bytes of the text;
 * the CIGAR entry's scan, in place in d_text_off; wfa_diff_write_kernel, a wave per pair in rounds of 64 ops, wave prefix sums giving
 * each op its first byte and its first bases -- a lane renders its own op where the text has at most 16 bytes, the whole wave sweeps
 * each longer op in turn, four bytes to a lane in groups aligned in d_text (one 4-byte store a group where d_text is 4-byte aligned),
 * so that no lane walks a count (KERNELS.md 4v).  Scratch lives in the context and is the CIGAR entry's; one fetch of 64 bytes of
 * counters per call crosses PCIe.  WFAHIP_DEBUG_TIMING=1 prints the passes' times to stderr. */
int  wfahip_diff_text_device(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap,
                             const void *d_seq_blob, uint64_t blob_bytes, const void *d_q_off, const void *d_q_len,
                             const void *d_t_off, const void *d_t_len, uint64_t n_pairs, int only_aligned,
                             void *d_text, uint64_t text_cap, void *d_text_off /* u64[n_pairs + 1] */, uint64_t *text_needed,
                             void *stream);

/* The difference string from 2-bit packed words, both strands.  For a flagged pair (d_q_rc[i] != 0) the record's coordinates and ops
 * count on the reverse-complemented query, which exists nowhere a caller can point to: this is the only compact product that names
 * its bases.  The letter of a code is "actg"[code] (wfa_altext_pk.hpp's letter, lower-cased like any other byte); base p of a flagged
 * query of len bases is the complement (code ^ 2) of forward base len - 1 - p.  The text equals, byte for byte, what
 * wfahip_diff_text_device writes for the same records and ops over the corresponding bytes.
 * d_rec / d_ops, the words, the offsets (u64), lengths (u32) and flags (u8 per pair, NULL = none set) as
 * wfahip_alignment_text_packed_device takes them, and with that entry's rules word for word: offsets may come in any order, repeat,
 * alias, and name a prefix of a longer sequence under another length or flag; the offsets of a pair that renders nothing (status not
 * OK, OPS_LEN 0, no op that renders a byte, no 'M' op under only_aligned) are never looked at; of a sequence that renders only words
 * in [woff, woff + wfahip_packed_words(len)) are read, no result depends on the bits of its last word beyond its last base or on its
 * pad word, and d_packed needs NO readable memory behind its n_words words.  The checks are that entry's: the ops lie in [0, ops_cap);
 * for both sequences woff <= n_words and wfahip_packed_words(len) <= n_words - woff; trimmed, 1 <= BEGIN, BEGIN - 1 <= END and END <=
 * the sequence's length; the bases consumed fit the windows.  d_text, d_text_off, *text_needed, text_cap, WFAHIP_ERR_OOM,
 * WFAHIP_ERR_BAD_ARG (d_text untouched, before the kernel that reads a word to write text is launched), n_pairs == 0, stream,
 * synchrony and wfahip_last_timing (untouched) are wfahip_diff_text_device's, word for word; no input is written.
 * WFAHIP_ERR_BAD_ARG before the context is dereferenced: a null ctx; with n_pairs > 0 a null d_rec, d_text_off, d_q_woff, d_q_len,
 * d_t_woff or d_t_len; a null d_ops with ops_cap > 0; a null d_packed with n_words > 0; a null d_text with text_cap > 0; n_pairs
 * beyond 0xFFFFFFF0.  Three passes: wfa_diff_pk_len_kernel, the scan, wfa_diff_pk_write_kernel -- wfa_diff_write_kernel over the
 * packed rows' reader, four letters a funnel shift and one v_perm_b32 (KERNELS.md 4v). */
int  wfahip_diff_text_packed_device(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap,
                                    const void *d_packed, uint64_t n_words, const void *d_q_woff, const void *d_q_len,
                                    const void *d_t_woff, const void *d_t_len, const void *d_q_rc /* u8 per pair, NULL = none */,
                                    uint64_t n_pairs, int only_aligned, void *d_text, uint64_t text_cap,
                                    void *d_text_off /* u64[n_pairs + 1] */, uint64_t *text_needed, void *stream);

/* Host only, no device, no context: the same bytes and offsets for a wfahip_results in host memory and the blob and arrays (the
 * words, offsets, lengths and flags) it was aligned from -- n_threads host threads over contiguous ranges of pairs, the same header
 * functions as the kernels.  The trimmed windows are r->qbegin / qend / tbegin / tend.  out is wfahip_cigar_text's struct: text holds
 * n_bytes bytes (NULL when n_bytes == 0), off n + 1 offsets, off[0] = 0 and off[n] = n_bytes; both are malloc'd and released with
 * wfahip_cigars_free.  r->n == 0 gives n = n_bytes = 0, text = NULL and off pointing at one 0.  WFAHIP_ERR_BAD_ARG (out zeroed, when
 * there is one) as wfahip_alignment_text / wfahip_alignment_text_packed: a null r or out; with r->n > 0 a null status, ops_off,
 * ops_len, offset or length array, and under only_aligned a null qbegin, qend, tbegin or tend; a null ops with n_ops > 0; a null
 * seq_blob with blob_bytes > 0 (a null packed with n_words > 0); a pair that fails a check of the device entry (with n_ops as
 * ops_cap). */
int  wfahip_diff_text(const wfahip_results *r, const uint8_t *seq_blob, uint64_t blob_bytes, const uint64_t *q_off,
                      const uint32_t *q_len, const uint64_t *t_off, const uint32_t *t_len, int only_aligned, int n_threads,
                      wfahip_cigars *out);
int  wfahip_diff_text_packed(const wfahip_results *r, const uint32_t *packed, uint64_t n_words, const uint64_t *q_woff,
                             const uint32_t *q_len, const uint64_t *t_woff, const uint32_t *t_len,
                             const uint8_t *q_rc /* NULL = none */, int only_aligned, int n_threads, wfahip_cigars *out);

/* The pileup: what a batch's alignments say about every base of the TARGET, counted where the ops and the sequences are.  Every
 * product above is per pair and leaves the GPU as text; a polisher, a consensus step, a variant screen or a coverage plot wants one
 * small record per target base, and the entries say already that offsets may repeat: one target may face fifty queries.  A pileup is
 * a caller-owned array of WFAHIP_PILE_WORDS = 8 u32 words for every base of a WINDOW [pile_at, pile_at + pile_n) of the target's
 * storage -- for the byte entries the byte index into the blob, for the packed entries the base index 16 * woff + p (the "bytes the
 * words stand for" of wfahip_align_batch_packed_rc).  32 bytes a base, whatever the depth:
 *     A, C, T, G     alignments that put that query base over this target base (an M or X column).  The code of a query base is the
 *                    packer's, (byte >> 1) & 3 of a byte among ACGTacgt -- hence the order A C T G
 *     OTHER          ... a query byte outside those eight letters (packed input has none)
 *     GAP            alignments in which this target base faces '-' (an I column)
 *     EXTRA          runs of query-only bases (D ops) that hang behind this base
 *     EXTRA_BASES    the bases of those runs
 * The rule (wfa_amd/csrc/wfa_pile.hpp, one source for the kernels and the host entries), per op word letter << 32 | count, with qs /
 * ts the bases the ops before it consumed inside the pair's windows and T0 the coordinate of the target window's first base (t_off +
 * the window's start for bytes, 16 * t_woff + it for words):
 *     M, X       column c < count: base P = T0 + ts + c gets + 1 in the word of query base qs + c.  Ops are taken at face value: an M
 *                column is not compared with the target, as in the difference string
 *     I          column c: base P = T0 + ts + c gets + 1 in GAP
 *     D          count > 0: one add of 1 to EXTRA and one of count to EXTRA_BASES at base P = T0 + max(ts, 1) - 1 -- the run hangs on
 *                the target base before it; a run in front of the window's first base shares base 0's counters (trimmed ranges begin
 *                and end with M, so that happens only untrimmed).  Nothing when the target's window is empty
 *     H, any other letter, count 0: nothing (H consumes query bases, as in the display rows)
 * An add happens only when pile_at <= P < pile_at + pile_n, at counts[(P - pile_at) * 8 + word].  The entries ADD and never clear:
 * the caller zeroes the array, and several batches, both strands or several calls accumulate into one pileup; a large reference is
 * tiled over calls or GPUs by its window, as the score matrix is by its strided output.  Adds are u32 and wrap; integer adds
 * commute, so the counters do not depend on scheduling.  A flagged query's base p is code ^ 2 of forward base len - 1 - p.
 * Which pairs and ops count is wfahip_alignment_text_device's (packed: wfahip_alignment_text_packed_device's), exactly, decided by
 * the same functions: only_aligned == 0 all ops over the whole sequences, only_aligned != 0 the first M op to the last over the windows
 * the record names; a pair whose status is not WFAHIP_PAIR_OK, whose OPS_LEN is 0 or that trimmed has no M op adds nothing and its
 * offsets are never looked at, nor are, in the packed entries, those of a pair whose ops have no column.  The checks are those entries'
 * too, in the same order for every pair that would count: the ops lie in [0, ops_cap); both sequences lie inside the blob (the words);
 * trimmed, 1 <= BEGIN, BEGIN - 1 <= END and END <= the sequence's length; the bases consumed fit the windows.  A failed check:
 * WFAHIP_ERR_BAD_ARG with the counters untouched, before the kernel that reads a sequence byte is launched.  Untrimmed, a batch with
 * the wf-adaptive pair whose ops consume one base more than the sequences hold is therefore refused: wfahip_check_alignments*'s
 * d_pass under WFAHIP_CHK_NO_ROWS, copied over the status column of a copy of the records, sets it aside.
 *
 * wfahip_pileup_device / wfahip_pileup_packed_device: d_rec / d_ops, the blob (the words), the arrays and the flags as
 * wfahip_diff_text_device / wfahip_diff_text_packed_device take them, with those entries' rules for pointers, stream (NULL = the
 * context's own) and synchrony; no input is written; only bytes (words) inside the sequences are read -- the query's under M and X
 * columns inside the window, the target's never.  d_counts: u32[8 pile_n], 4-byte aligned, the caller's.  The window may lie anywhere,
 * also outside the blob: it then receives nothing.  *n_piled (if non-NULL) receives the number of pairs whose ops were swept -- the
 * pairs with a column, whether or not one of them falls into the window -- from the one 64-byte counter fetch of the call.  pile_n ==
 * 0 or n_pairs == 0 returns WFAHIP_OK with *n_piled = 0 and touches nothing.  WFAHIP_ERR_BAD_ARG before the context is dereferenced:
 * a null ctx; with n_pairs > 0 a null d_rec, offset or length array; a null d_ops with ops_cap > 0; a null blob (words) of non-zero
 * size; a null d_counts with pile_n > 0; pile_n beyond 2^61 / 8; n_pairs beyond 0xFFFFFFF0.  wfahip_last_timing is not touched.
 * Two passes (wfa_cigar.hip): wfa_pile_len_kernel / wfa_pile_pk_len_kernel, the display rows' length pass -- range, sums, checks --
 * without its offsets and its scan, one atomic a wave counting the pairs; wfa_pile_kernel / wfa_pile_pk_kernel, a wave per pair in
 * rounds of 64 ops with the rows' table in LDS: a D op's two adds are its own lane's, the target-consuming columns are swept by target
 * base, consecutive lanes on consecutive bases, each finding its op by a search over the table's target starts, and every column is
 * one atomic add without a return; no lane walks a count, and only the part of a pair inside the window is walked (KERNELS.md 4w).
 * WFAHIP_DEBUG_TIMING=1 prints the passes' times to stderr.
 *
 * wfahip_pileup / wfahip_pileup_packed: host only, no device, no context, the same header functions: n_threads host threads over
 * contiguous ranges of pairs, adding with relaxed atomic adds because pairs share targets.  counts is the caller's, 8 pile_n words.
 * WFAHIP_ERR_BAD_ARG (counts untouched) as wfahip_diff_text / wfahip_diff_text_packed -- a null r; with r->n > 0 a null status,
 * ops_off, ops_len, offset or length array, and under only_aligned a null qbegin, qend, tbegin or tend; a null ops with n_ops > 0; a
 * null seq_blob (packed) of non-zero size; a pair that fails a check of the device entry (with n_ops as ops_cap) -- and for a null
 * counts with pile_n > 0 and pile_n beyond 2^61 / 8.  r->n == 0 or pile_n == 0: WFAHIP_OK, *n_piled = 0, nothing touched. */
#define WFAHIP_PILE_WORDS 8
enum { WFAHIP_PILE_W_A = 0, WFAHIP_PILE_W_C, WFAHIP_PILE_W_T, WFAHIP_PILE_W_G, WFAHIP_PILE_W_OTHER, WFAHIP_PILE_W_GAP, WFAHIP_PILE_W_EXTRA,
       WFAHIP_PILE_W_EXTRA_BASES };
int  wfahip_pileup_device(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap, const void *d_seq_blob,
                          uint64_t blob_bytes, const void *d_q_off, const void *d_q_len, const void *d_t_off, const void *d_t_len,
                          uint64_t n_pairs, int only_aligned, uint64_t pile_at, uint64_t pile_n, void *d_counts /* u32[8 pile_n] */,
                          uint64_t *n_piled /* may be NULL */, void *stream);
int  wfahip_pileup_packed_device(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap, const void *d_packed,
                                 uint64_t n_words, const void *d_q_woff, const void *d_q_len, const void *d_t_woff, const void *d_t_len,
                                 const void *d_q_rc /* u8 per pair, NULL = none */, uint64_t n_pairs, int only_aligned, uint64_t pile_at,
                                 uint64_t pile_n, void *d_counts /* u32[8 pile_n] */, uint64_t *n_piled /* may be NULL */, void *stream);
int  wfahip_pileup(const wfahip_results *r, const uint8_t *seq_blob, uint64_t blob_bytes, const uint64_t *q_off, const uint32_t *q_len,
                   const uint64_t *t_off, const uint32_t *t_len, int only_aligned, int n_threads, uint64_t pile_at, uint64_t pile_n,
                   uint32_t *counts /* 8 pile_n */, uint64_t *n_piled /* may be NULL */);
int  wfahip_pileup_packed(const wfahip_results *r, const uint32_t *packed, uint64_t n_words, const uint64_t *q_woff, const uint32_t *q_len,
                          const uint64_t *t_woff, const uint32_t *t_len, const uint8_t *q_rc /* NULL = none */, int only_aligned,
                          int n_threads, uint64_t pile_at, uint64_t pile_n, uint32_t *counts /* 8 pile_n */,
                          uint64_t *n_piled /* may be NULL */);

/* The check: is each alignment consistent with its sequences, what does it cost, and which pairs are not?  One pass over records,
 * ops and sequences where they lie; per pair WFAHIP_CHK_WORDS = 8 u32 words -- FLAGS, COST, Q_USED, T_USED, N_BAD, FIRST_BAD, 0, 0 --
 * and, if asked for, a status for the stages behind.  The flags state what IS, not what is wrong: the reference's own results raise
 * NO_M, Q_OVER / T_OVER, COST_UNDER and M_DIFFERS now and then (short noisy pairs under an aggressive wf-adaptive; KERNELS.md 4u), and
 * this library returns what the reference returns.  A caller picks the flags it minds with flag_mask.
 * The rule (wfa_amd/csrc/wfa_check.hpp, one source for the kernels and the host entries), in this order:
 *  1. status not WFAHIP_PAIR_OK: all eight words 0; nothing else of the pair is read -- its record may hold stale words, its offsets
 *     are never looked at;
 *  2. OPS_RANGE: OPS_LEN > ops_cap or OPS_OFF > ops_cap - OPS_LEN.  FLAGS = OPS_RANGE | NO_ROWS | NO_ROWS_TRIMMED, the other words 0,
 *     no op is read;
 *  3. over all ops: LETTER, an op letter outside M X I D H; ZERO, an op with count 0; UNMERGED, two neighbouring ops of one letter;
 *     NO_M, no 'M' op (an empty op list has none);
 *  4. Q_USED / T_USED: the query / target bases the ops consume (M X: both, I: target, D H: query, any other letter: none).  COST:
 *     x * count for X, o + e * count for I, D and H, 0 for everything else.  Each word is min(true value, 0xFFFFFFFF); the true values
 *     are carried wide enough that a count of 0xFFFFFFFF under a penalty of 0xFFFFFFFF does not wrap;
 *  5. SEQ_RANGE: a sequence with off > blob_bytes or len > blob_bytes - off (words: woff > n_words or wfahip_packed_words(len) >
 *     n_words - woff).  No sequence byte of the pair is read; N_BAD = 0, FIRST_BAD = 0xFFFFFFFF;
 *  6. Q_OVER / Q_UNDER / T_OVER / T_UNDER: the bases consumed against the sequence's length;
 *  7. only the M and X columns whose query index is < q_len and whose target index is < t_len are compared, byte with byte as the
 *     reference compares them (packed input: code with code; base p of a flagged query is code ^ 2 of forward base len - 1 - p).
 *     M_DIFFERS: an M column whose two bytes differ.  X_EQUAL: an X column whose bytes are equal.  N_BAD counts such columns
 *     (saturating); FIRST_BAD is min(index of the first among all columns of the untrimmed rows, 0xFFFFFFFE), 0xFFFFFFFF without one;
 *  8. NO_ROWS / NO_ROWS_TRIMMED: the checks of wfahip_alignment_text_device (packed: of wfahip_alignment_text_packed_device) with
 *     only_aligned = 0 / 1 fail for this pair -- decided by the functions those entries call;
 *  9. only when p->global_alignment != 0: COST_OVER, the true cost > SCORE; COST_UNDER, the true cost < SCORE (the reference's merge of
 *     two separately opened gaps into one op);
 * 10. STAT_ALIGN_LEN / STAT_MATCHES / STAT_GAPS / STAT_GAP_REGIONS: the record's field differs from process() recomputed over the ops
 *     (wfa_cigar.go:171-211): u32 wrapping sums from the first M op to the last -- without an M op over op 0 alone, as the Go loop
 *     behaves --, H counted in the length and not in the gaps. */
#define WFAHIP_CHK_WORDS 8
enum { WFAHIP_CHK_W_FLAGS = 0, WFAHIP_CHK_W_COST, WFAHIP_CHK_W_Q_USED, WFAHIP_CHK_W_T_USED, WFAHIP_CHK_W_N_BAD, WFAHIP_CHK_W_FIRST_BAD };
#define WFAHIP_CHK_OPS_RANGE        (1u << 0)
#define WFAHIP_CHK_LETTER           (1u << 1)
#define WFAHIP_CHK_ZERO             (1u << 2)
#define WFAHIP_CHK_UNMERGED         (1u << 3)
#define WFAHIP_CHK_NO_M             (1u << 4)
#define WFAHIP_CHK_SEQ_RANGE        (1u << 5)
#define WFAHIP_CHK_Q_OVER           (1u << 6)
#define WFAHIP_CHK_Q_UNDER          (1u << 7)
#define WFAHIP_CHK_T_OVER           (1u << 8)
#define WFAHIP_CHK_T_UNDER          (1u << 9)
#define WFAHIP_CHK_M_DIFFERS        (1u << 10)
#define WFAHIP_CHK_X_EQUAL          (1u << 11)
#define WFAHIP_CHK_NO_ROWS          (1u << 12)
#define WFAHIP_CHK_NO_ROWS_TRIMMED  (1u << 13)
#define WFAHIP_CHK_COST_OVER        (1u << 14)
#define WFAHIP_CHK_COST_UNDER       (1u << 15)
#define WFAHIP_CHK_STAT_ALIGN_LEN   (1u << 16)
#define WFAHIP_CHK_STAT_MATCHES     (1u << 17)
#define WFAHIP_CHK_STAT_GAPS        (1u << 18)
#define WFAHIP_CHK_STAT_GAP_REGIONS (1u << 19)
#define WFAHIP_CHK_ALL              ((1u << 20) - 1u)

/* wfahip_check_alignments_device: records, ops, blob and the four arrays as wfahip_alignment_text_device takes them, all device
 * addresses on the context's GPU that stay the caller's; no input is written.  d_chk receives 8 n_pairs u32 words (two 16-byte stores
 * a pair where d_chk is 16-byte aligned), d_pass -- if non-NULL -- n_pairs int32: the record's status when that is not OK, else
 * WFAHIP_PAIR_OK when FLAGS & flag_mask == 0, else WFAHIP_PAIR_CHECK_FAILED.  wfahip_select_pairs_device takes d_pass as its d_status
 * unchanged; copied over the status column of a copy of the records it makes the text entries render the remaining pairs.  Nothing
 * beyond those words and statuses is written.  *n_flagged (if non-NULL) receives the number of OK pairs with FLAGS & flag_mask != 0:
 * one 64-byte fetch of a counter in the context, the only thing that crosses PCIe.  A bad pair is never a call error here: it is a
 * flag.  Only bytes (words) inside the sequences are read: d_seq_blob and d_packed need no readable memory behind their
 * ends.  WFAHIP_ERR_BAD_ARG before the context is dereferenced: a null ctx, p or d_chk; with n_pairs > 0 a null
 * d_rec, offset or length array; a null d_ops with ops_cap > 0; a null blob (words) with a non-zero size; n_pairs beyond 0xFFFFFFF0.
 * Then the params are checked as wfahip_align_batch checks them.  n_pairs == 0 returns WFAHIP_OK with *n_flagged = 0 and touches
 * nothing.  stream = hipStream_t (NULL = the context's own).  Synchronous.  wfahip_last_timing is not touched.
 * One kernel (wfa_cigar.hip: wfa_check_kernel, wfa_check_pk_kernel): a wave per pair in rounds of 64 ops, the flags from ballots and a
 * neighbour compare, the display-row kernels' prefix sums and column sweep with a compare where they store; no scan, nothing
 * variable-length is written; one atomic a wave feeds the counter (KERNELS.md 4u).  WFAHIP_DEBUG_TIMING=1 prints the kernel's time. */
int  wfahip_check_alignments_device(wfahip_ctx *ctx, const wfahip_params *p, const void *d_rec, const void *d_ops, uint64_t ops_cap,
                                    const void *d_seq_blob, uint64_t blob_bytes, const void *d_q_off, const void *d_q_len,
                                    const void *d_t_off, const void *d_t_len, uint64_t n_pairs, uint32_t flag_mask,
                                    void *d_chk /* u32[8 n_pairs] */, void *d_pass /* int32[n_pairs], may be NULL */,
                                    uint64_t *n_flagged /* may be NULL */, void *stream);
/* The same over 2-bit packed words, both strands: inputs as wfahip_alignment_text_packed_device takes them (d_q_rc: u8 per pair, NULL
 * = none set). */
int  wfahip_check_alignments_packed_device(wfahip_ctx *ctx, const wfahip_params *p, const void *d_rec, const void *d_ops, uint64_t ops_cap,
                                           const void *d_packed, uint64_t n_words, const void *d_q_woff, const void *d_q_len,
                                           const void *d_t_woff, const void *d_t_len, const void *d_q_rc /* NULL = none */,
                                           uint64_t n_pairs, uint32_t flag_mask, void *d_chk, void *d_pass, uint64_t *n_flagged,
                                           void *stream);
/* Host only, no device, no context: the same words, statuses and count for a wfahip_results in host memory (n_ops as ops_cap; the
 * record's fields are r's arrays) and the blob (words) and arrays it was aligned from, n_threads host threads over contiguous ranges
 * of pairs, the same header functions as the kernels.  chk is the caller's, 8 r->n words; pass (r->n statuses) and n_flagged may be
 * NULL.  WFAHIP_ERR_BAD_ARG: a null r, p or chk; with r->n > 0 a null field array of r, offset or length array; a null ops with
 * n_ops > 0; a null blob (words) with a non-zero size; r->n beyond 0xFFFFFFF0.  Then the params as wfahip_align_batch checks them. */
int  wfahip_check_alignments(const wfahip_results *r, const wfahip_params *p, const uint8_t *seq_blob, uint64_t blob_bytes,
                             const uint64_t *q_off, const uint32_t *q_len, const uint64_t *t_off, const uint32_t *t_len,
                             uint32_t flag_mask, int n_threads, uint32_t *chk /* 8 r->n */, int32_t *pass /* may be NULL */,
                             uint64_t *n_flagged /* may be NULL */);
int  wfahip_check_alignments_packed(const wfahip_results *r, const wfahip_params *p, const uint32_t *packed, uint64_t n_words,
                                    const uint64_t *q_woff, const uint32_t *q_len, const uint64_t *t_woff, const uint32_t *t_len,
                                    const uint8_t *q_rc /* NULL = none */, uint32_t flag_mask, int n_threads, uint32_t *chk,
                                    int32_t *pass, uint64_t *n_flagged);

/* One pair at a time behind the batch: a caller that loops over pairs like the reference's CLI
 * (wfa-go/wfa-go.go:166-178: one Align per ">"/"<" record) submits each pair -- the bytes are copied, the call returns
 * at once with the pair's ticket (0, 1, 2, ... since the last collect) -- and collects all results with ONE batch
 * alignment: out->...[ticket] is the result of that submission.  Same thread rule as every other call on a context. */
int      wfahip_submit(wfahip_ctx *ctx, const uint8_t *q, uint32_t n, const uint8_t *t, uint32_t m, uint64_t *ticket);

/* Aligner.Align (wfa.go:196) for ONE pair, without the batch plumbing: no offset arrays in, no malloc'd result arrays
 * out.  rec receives the pair's record (WFAHIP_REC_WORDS u32: status, score, region, statistics, op count; OPS_OFF = 0),
 * ops the CIGAR ops (op<<32 | n, forward order, merged; capacity ops_cap entries), *n_ops their number.  If ops_cap is
 * too small the call returns WFAHIP_ERR_OOM with *n_ops = the capacity needed (at most n + m + 2).  Per-pair failures
 * are statuses in rec[WFAHIP_REC_STATUS] (EMPTY / TOO_LONG), like the batch entry.  A pair whose shape allows it (global,
 * penalties of a shape the register-ring kernels are built for -- x : o+e : e = 2:4:1 (4/6/2), 1:3:1, 1:2:1, 2:3:1, 2:2:1 or
 * 3:3:1 --, both sequences within ~30 kbp) takes ONE kernel launch and no copy -- a wave with a lane per
 * diagonal reads the sequences from, and writes record and CIGAR to, a page-locked block mapped into the GPU's address
 * space, and walks its own backtrace -- 0.144 ms for a 1 kbp pair as the round-4 driver measured it (round 3: 0.29;
 * wfahip_align_batch with n_pairs = 1: 0.45); every other pair, and one whose band leaves 64 diagonals, goes through that
 * entry.  Same results either way.
 * A caller that CAN batch should: a batch aligns ~55 million pairs a second, this call seven thousand. */
int      wfahip_align_pair(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *q, uint32_t n, const uint8_t *t, uint32_t m,
                           uint32_t *rec, uint64_t *ops, uint64_t ops_cap, uint64_t *n_ops);
uint64_t wfahip_pending(const wfahip_ctx *ctx);
int      wfahip_collect(wfahip_ctx *ctx, const wfahip_params *p, wfahip_results *out);

/* A set of contexts, one per GPU, behind one call (wfahip_create(device_ids, n_devices)).
 * wfahip_align_batch_multi cuts the batch into contiguous shards of pairs balanced by sequence bytes, aligns every
 * shard on its own GPU from its own host thread (alignments share no state: one Aligner per goroutine in the
 * reference, wfa.go:73-78) and merges the results in pair order.  device_ids == NULL: devices 0 .. n_devices-1
 * (n_devices <= 0: every device).  The same id may appear more than once (several contexts on one GPU). */
typedef struct wfahip_multi wfahip_multi;
int         wfahip_create_multi(const int *device_ids, int n_devices, wfahip_multi **out);
void        wfahip_destroy_multi(wfahip_multi *m);
int         wfahip_multi_size(const wfahip_multi *m);
wfahip_ctx *wfahip_multi_ctx(wfahip_multi *m, int i); /* for wfahip_set_option / wfahip_last_timing; owned by m */
int         wfahip_align_batch_multi(wfahip_multi *m, const wfahip_params *p, const uint8_t *seq_blob,
                                     uint64_t blob_bytes, const uint64_t *q_off, const uint32_t *q_len,
                                     const uint64_t *t_off, const uint32_t *t_len, uint64_t n_pairs,
                                     wfahip_results *out);

int  wfahip_last_timing(const wfahip_ctx *ctx, wfahip_timing *out);

/* Options (optional; results never depend on them).
 *
 * PUBLIC keys -- always accepted:
 *   "census"  0|1          count the wavefront words every pair stores (WFAHIP_REC_CELLS, timing.cells_stored)     default 0
 *   "learn"  0|1           long pairs start on the arena level the previous call of the same kind needed            default 1
 *   "mem_limit"  bytes     device memory the context may plan with (0 = all of it)
 *   "arena_budget_pct"     share of that memory the long-pair arenas may take                                       default 80
 *   "autopack"  0|1        the host entry 2-bit packs ACGT-only batches before the upload                           default 1
 *   "pair_fast", "pair_lds"   wfahip_align_pair's path (described at the end of the list below)
 *
 * DEBUG keys -- every other key below: a routing experiment, a test aid or the knob of one kernel family.  They are refused
 * with WFAHIP_ERR_UNSUPPORTED unless WFAHIP_DEBUG=1 is set in the environment of the process (tests/conftest.py, bench.py
 * --opt and the scripts under scripts/ set it).  Some change what is SAFE, not only what is fast ("team_strict" 0,
 * "fail_pass"); none belongs in a deployment.
 *   "blk"  16 | 8 | 0      blocked register-window forward kernel, lanes per pair (0 = off)       default 16
 *   "reg", "packed"  0|1   allow the strided register-window / LDS-ring forward kernels           default 1
 *   "packed_arena_bytes"   per-pair arena of the sub-wave pipeline (0 = automatic)
 *   "chunk_pairs", "packed_waves_per_cu", "overlap"   chunking of the sub-wave pipeline
 *   "tail_overlap"  0|1    retry passes run beside the first pass's backtrace kernel             default 1
 *   "pilot"  0|1           wf-adaptive off, >= 65 536 pairs of >= 200 bases: 4 096 pairs go first and decide whether
 *                          the rest starts on the 64-diagonal kernel, on the 256-diagonal one, or on the
 *                          generic kernel                                                          default 1
 *   "blk_batch"  0..8      short reads: a group of the blocked kernel stages several pairs per refill
 *                          (1 = as many as spreads the chunk evenly, at most 8; 2..8 = that many)  default 1
 *   "bt_stream"  n         n waves of the first pass's launch backtrace finished pairs while the other
 *                          waves are still aligning (0 = backtrace kernel after the forward kernel)  default 96
 *   "bt_stream_min"        ... for chunks of at least this many pairs                              default 393216
 *   "bt_stream_single" 0|1 switches the streamed backtrace on (any number of chunks); off by default since round 2:
 *                          a backtrace kernel per chunk is faster now (3e6 x 1 kbp pairs: 65.2 vs 70.5 ms)        default 0
 *   "bt_stream_wait_us"    a streaming wave that waits longer than this for a finished pair leaves the
 *                          rest to the backtrace kernel that follows the launch                     default 20000
 *   "blk_narrow"  0|1      reads under 200 bases start with eight pairs per wave (8 lanes, 32 diagonals each);
 *                          what outgrows that retries on the 16-lane instance                         default 1
 *   "blk_wide"  0|1        pairs whose band leaves the 64-diagonal window retry on the same kernel with a
 *                          wave per pair (256 diagonals) before the generic kernel takes them       default 1
 *   "wide"  0|1|3          the pairs of a semi-global batch whose reads have up to 2 047 bases start on wfa_wide_kernel (round 6: a
 *                          workgroup per pair, the rows in 16-bit LDS rings of any width; two launches per chunk under wf-adaptive --
 *                          wide rows, then the narrow tail from a checkpoint) when there are at least "wide_min_pairs" of them
 *                          (default 64), whatever else the batch holds: longer pairs take the ladder.  3: one launch per chunk;
 *                          0: on the generic ladder.  "wide_max_len" below 2 047: the batch's longest read decides for the whole
 *                          batch, as before there were length classes                                               default 1
 *   "wide_bin_min_pairs"   batches of at least this many pairs are cut into length classes on the device (wfahip_wide_class_bounds;
 *                          a launch per class, sized by the class's own longest read; a class of fewer than "wide_min_pairs"
 *                          pairs rides with the next larger one); smaller batches are one class sized by min(longest read,
 *                          2 047) and the kernel hands the longer pairs on                                        default 4096
 *   "wide_classes"  0|1    0: a batch that is cut into classes runs as ONE class sized by its longest classed read (A/B runs,
 *                          tests)                                                                                   default 1
 *   "wide_waves"  0|1|4    waves per pair in its first launch: 0 = by the rings' size (four above 12 KB)          default 0
 *   "matrix_tile_cells"    wfahip_score_matrix: cells per tile (0 = automatic: 4 194 304 global, 262 144 semi-global; tests force
 *                          small tiles so that the tiles split rows and columns)                                default 0
 *   "score_long_min"       wfahip_score_batch / wfahip_score_matrix: global pairs (cells) of reads beyond 2 047 bases run on
 *                          wfa_score_long_kernel when a call holds at least this many of them; fewer take the full path (such a launch
 *                          fills a sixteenth of the SIMDs, and the arena it saves is a few MB; tests set 1)                  default 64
 *   "score_long_window_words"  packed words of each sequence such a pair keeps in LDS (16..4096, a multiple of 4; results do not
 *                          depend on it: a cell outside the window reads global memory)                                 default 256
 *   "arena_bytes_per_slot", "slots", "threads_per_pair"   generic kernel (one workgroup per pair)
 *   "prepack"  0|1         the sequences of a chunk are 2-bit packed by a kernel of their own before the 16-lane forward
 *                          kernel, whose refill then is one round of loads (forward pass -2 %, packing kernel +4 %)   default 0
 *   "narrow_long"  0|1     reads of any length start on the 8-lanes-per-pair instance (experiment: the refills of the
 *                          hand-over cost more than the narrow steps save)                                            default 0
 *   "census"  0|1          count the wavefront words every pair stores (WFAHIP_REC_CELLS, timing.cells_stored: the roofline
 *                          accounting of bench.py); instrumentation, 4 % of the forward pass on 1 kbp pairs.  The kernels for
 *                          long / semi-global pairs always count                                                default 0
 *   "learn"  0|1            long pairs (team kernel): start on the arena level by which 90 % of the long pairs of the
 *                          previous call of the same kind had finished, instead of climbing from the smallest      default 1
 *   "team_min_len"         pairs at least this long use the team kernel (0 = never)              default 8192
 *   "team_wgs", "team_solo_max"   workgroups per team (0 = automatic), widest row done by one workgroup
 *   "team_wave"                   1 (default): rows of at most 64 diagonals are stepped by one wave out of an LDS ring
 *                                 (team kernel and the one-workgroup-per-pair kernel: wfa_wave.hpp)
 *   "team_strict"                 1 (default): every team barrier carries an agent-scope release (L2 write-back + wait).
 *                                 0: no release -- 10 % faster on 100 kbp pairs and NOT safe: a row word can be read before
 *                                 its write-through has landed (measured; wfa_team.hpp)
 *   "arena_poison"                tests: fill the arena with a pattern before every forward launch (no kernel may read a word
 *                                 it did not write in this launch)
 *   "duo_pk"  0|1                 1 (default): wfa_duo_kernel holds its rings as 16-bit pairs; 0: its 32-bit-ring reference
 *                                 wfa_duo32_kernel (tests and A/B runs: both write the same arena words, byte for byte)
 *   "duo_claim"  1..8             wfa_duo_kernel: the most fetches a wave claims with one atomic on the pair queue's head word; above 1 a
 *                                 wave also starts with eight entries of its own.  1: one fetch per atomic from entry 0 on, as before
 *                                 there were blocks (tests and A/B runs: results do not depend on it)                    default 4
 *   "team_paged"  0|1             1 (default): the teams of the long-pair kernel share ONE pool of arena pages -- a pair holds what it
 *                                 needs, up to eight teams run at once -- instead of a slot each sized for the worst pair
 *   "team_xcd"  0|1|2             teams of one XCD's 32 CUs (1); 2 (default): ... and a team that finds all its workgroups on one
 *                                 XCD keeps its rows in that XCD's L2 (checked at run time; any other placement: the memory-side protocol)
 *   "long"  0|1                   1 (default): global pairs longer than "long_min_len" (4 000) bases, penalties shaped 4/6/2, take the
 *                                 sub-wave kernels with sliding 2-bit sequence windows in LDS (any read length); 0: as in round 3
 *   "long_first"  0|11..15        which of those instances a batch starts on: 0 = by batch size (up to six pairs per SIMD, 6 144: a
 *                                 wave per pair with two diagonals per lane; else four pairs per wave)
 *   "long_window_words"           packed words of each sequence a pair keeps in LDS (default 240 = 3 840 bases; 64..4096)
 *   "long_wave_bt"  0|1|2         backtrace of those pairs by a wave per pair (1: for chunks of at most "long_wave_bt_pairs" pairs --
 *                                 default twenty per CU, 5 120; 2: always; 0: never)
 *   "long_mid_lone"  0|1          1 (default): long pairs handed on for their band, when they are at most six per SIMD, go to the
 *                                 wave-per-pair instance with two diagonals per lane (128 diagonals); 0: two pairs per wave
 *   "pair_fast"  0|1|2|3          wfahip_align_pair: 1 (default) one launch of the lone-pair instance (the wave walks its own
 *                                 backtrace); 3 / 2: round 3's one- / two-launch paths; 0: the batch entry
 *   "pair_lds"  0|1               1 (default): that instance keeps the pair's arena rows in LDS (160 KB: scores up to ~1 240 at
 *                                 penalties 4/6/2; a pair that needs more is re-run with the rows in global memory, and the next 64
 *                                 calls start there); 0: rows in global memory */
int  wfahip_set_option(wfahip_ctx *ctx, const char *key, int64_t value);

/* Debug / parity aid: align ONE pair and return every stored wavefront row.  rows[] receives
 * n_rows descriptors {score, lo, width, offset into words}; words[] holds, per row, the M, I and D
 * raw words (offset<<3|tag, 0 = absent; wfa_wavefront.go:93) for k = lo .. lo+width-1,
 * 3*width words per row.  Caller frees both with wfahip_free. */
typedef struct { uint32_t score; int32_t lo; uint32_t width; uint64_t word_off; } wfahip_row;
int  wfahip_debug_wavefronts(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *q, uint32_t n,
                             const uint8_t *t, uint32_t m, wfahip_row **rows, uint64_t *n_rows,
                             uint32_t **words, uint64_t *n_words, wfahip_results *res);
void wfahip_free(void *p);

/* Debug / parity aid: the compact backtrace arena of pair `pair` (an index of the most recent batch, inside its first
 * chunk) exactly as the first-pass sub-wave forward kernel left it in HBM, + the pair's meta words {status, final
 * score, end offset, cells}.  One word per diagonal and score: bit 0 the M cell took the insertion's offset, bit 1 it
 * took the mismatch's (which wins ties, wfa.go:657-693; neither: the deletion's), bit 2 the D cell is a DeleteExt
 * (else DeleteOpen), bit 3 the I cell is an InsertExt (else InsertOpen), bits 4-31 the pre-extension offset backTrace
 * recomputes (wfa.go:766-817); a seed of initComponents has offset 0 and bit 0 = Match / bit 1 = Mismatch.  Whether a
 * cell exists is not recorded (the walk only visits cells a stored decision names).  *fmt = layout: 1 = 64 words per
 * score index (score / gcd), diagonal k at slot k & 63; 3 = tiles of 8 score indices x 64 diagonals,
 * [(k & 63) / 4][index & 7][k & 3]; 4 = 256 words per index, slot k & 255; 5 = 32 words per index, slot k & 31; 6 = 128 words
 * per index, slot k & 127; 8 = 32 HALFWORDS per index (wfa_lane_kernel); 10 = halfwords, groups of four diagonals two by two
 * (wfa_duo_kernel, round 6): [(k & 63) / 8][index / 8][(k / 4) & 1][index & 7][k & 3] with n_words / 32 indices per pair of groups
 * (7: fmt 3 with halfwords, its tiled predecessor; 9: one group after the other, [(k & 63) / 4][index][k & 3]).
 * Slots the kernel never wrote hold stale bytes.  Caller frees *words with wfahip_free. */
/* Round 5: the same for a pair on wfa_teamc_kernel (wide wavefronts: option team_wgs = the team's size must be set): every row as
 * the kernel leaves it in the arena -- ONE backtrace word per diagonal (the pre-extension offset backTrace recomputes,
 * wfa.go:766-817, shifted left by four over the decisions of next(): bit 0 the M cell took the insertion's offset, bit 1 the
 * mismatch's, bit 2 the D cell is a DeleteExt, bit 3 the I cell is an InsertExt; offset 0 = a seed of initComponents, bit 0
 * Match / bit 1 Mismatch), rows[i].width words at rows[i].word_off, restricted to the band wf-adaptive kept. */
int  wfahip_debug_team_compact(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *q, uint32_t n, const uint8_t *t, uint32_t m,
                               wfahip_row **rows, uint64_t *n_rows, uint32_t **words, uint64_t *n_words, wfahip_results *res);
int  wfahip_debug_compact_arena(wfahip_ctx *ctx, uint64_t pair, uint32_t **words, uint64_t *n_words, uint32_t *fmt,
                                uint32_t *meta4);

/* Debug / test aid, host only (no device, no context): what wfahip_score_batch hands wfa_score_long_kernel for a batch.  The global
 * pairs with a read beyond 2 047 bases (neither sequence empty or over WFAHIP_MAX_SEQ_LEN) are 2-bit packed, pair after pair in batch
 * order, query then target, in wfahip_pack_pairs' layout: *words (*n_words of them).  *table lists the *n_listed of them without a
 * byte outside ACGT, eight words each: {query word offset lo, hi, query length, pair index, target word offset lo, hi, target
 * length, 0}.  Caller frees *words and *table with wfahip_free. */
int  wfahip_debug_score_long_list(const uint8_t *seq_blob, const uint64_t *q_off, const uint32_t *q_len, const uint64_t *t_off,
                                  const uint32_t *t_len, uint64_t n_pairs, uint32_t **words, uint64_t *n_words, uint32_t **table,
                                  uint64_t *n_listed);

/* Debug / test aid: the same buffer and table as the LAST wfahip_score_batch_device call on ctx built them on the device
 * (wfa_score_plan_kernel, wfa_score_pack_kernel, wfa_score_list_kernel), copied to the host: word for word what
 * wfahip_debug_score_long_list returns for the same batch.  *n_words == 0 (and NULL arrays) when that call ran no long pairs on
 * wfa_score_long_kernel; valid until the next score call on ctx.  Caller frees *words and *table with wfahip_free. */
int  wfahip_debug_score_device_list(wfahip_ctx *ctx, uint32_t **words, uint64_t *n_words, uint32_t **table, uint64_t *n_listed);

/* Debug / test aid, refused with WFAHIP_ERR_UNSUPPORTED unless WFAHIP_DEBUG=1 is in the environment: the byte-input packing pass
 * (wfa_prepack_kernel) alone, over device-resident pairs.  Slot i of the n is that of pair d_work[i] (d_work: n device uint32, or
 * NULL: pair i), 4 + 2 * seq_words words: {q_len, t_len, status, 0, seq_words query words, seq_words text words} -- 16 bases a word,
 * the first in the low bits, code (byte >> 1) & 3, 0 behind a sequence's end; status 0xFFFFFFFF (to be aligned), 1 (an empty
 * sequence), 2 (too long), 102 (longer than the slot), 100 (a byte outside ACGT).  Only slots of status 0xFFFFFFFF and 100 hold
 * words.  ppw (1 .. 32): pairs a wave packs.  slots: host memory for n * (4 + 2 * seq_words) words; a word the kernel did not
 * store reads 0xA5A5A5A5. */
int  wfahip_debug_prepack(wfahip_ctx *ctx, const void *d_seq_blob, const void *d_q_off, const void *d_q_len, const void *d_t_off,
                          const void *d_t_len, const void *d_work, uint64_t n, uint32_t seq_words, uint32_t ppw, uint32_t *slots);

/* The length classes semi-global batches are cut into before wfa_wide_kernel takes them: upper bounds of max(q_len, t_len),
 * strictly ascending, the last one 2 047.  Host only, no device.  Fills bounds[0 .. min(cap, count)) (bounds may be NULL when
 * cap is 0) and returns the count. */
int  wfahip_wide_class_bounds(uint32_t *bounds, int cap);

/* Debug / test aid: the plan kernels alone (wfa_wide_plan_*: count per tile, scan, scatter) over host length arrays.  *ids:
 * n_pairs pair indices -- per class the ascending list of its pairs, class after class, then the ascending list of the pairs
 * the wide kernel is not offered (both sequences non-empty and within WFAHIP_MAX_SEQ_LEN, the longer one beyond 2 047 bases; a
 * pair with an empty or over-long sequence is of the smallest class).  counts[c] / longest[c] for each class c of
 * wfahip_wide_class_bounds (longest: over the class's pairs with two valid sequences, 0 if none); *n_ladder: the length of the
 * last list.  Caller frees *ids with wfahip_free. */
int  wfahip_debug_wide_plan(wfahip_ctx *ctx, const uint32_t *q_len, const uint32_t *t_len, uint64_t n_pairs, uint32_t **ids,
                            uint64_t *counts, uint32_t *longest, uint64_t *n_ladder);

/* Synthetic input generator (host): the seeded dataset spec of DESIGN.md (mirrors what
 * WFA's generate_dataset, used by README.md:298-306, produces: random ACGT pattern of length
 * `length`, text = pattern with round(length*error_rate) random edits).  Pair i uses
 * splitmix64(seed ^ (first_index+i)*0x9E3779B97F4A7C15).  query = pattern, target = text
 * (wfa-go/wfa-go.go:166-178).  blob must hold n_pairs*stride bytes with
 * stride = wfahip_gen_stride(length, error_rate); offsets/lengths arrays hold n_pairs entries. */
uint64_t wfahip_gen_stride(uint32_t length, double error_rate);
int      wfahip_generate_pairs(uint64_t seed, uint64_t first_index, uint64_t n_pairs, uint32_t length,
                               double error_rate, int n_threads, uint8_t *blob, uint64_t *q_off,
                               uint32_t *q_len, uint64_t *t_off, uint32_t *t_len);

/* The same dataset generated on the device: byte for byte what wfahip_generate_pairs writes
 * into the sequences (padding bytes between sequences are not defined), with nothing crossing PCIe.  d_blob must hold
 * n_pairs * wfahip_gen_stride(length, error_rate) + 16 bytes, the other arrays n_pairs entries; all device addresses
 * on the context's GPU.  stream = hipStream_t (NULL = the context's own); returns when the data is there.
 * WFAHIP_ERR_UNSUPPORTED when a pair's text does not fit the LDS it is edited in (length + edits > 160 KB). */
/* Diagnostics for the bench (round 5): the shader clock UNDER LOAD.  Launches a short kernel that keeps every SIMD issuing
 * dependent vector instructions (~0.3 ms) and compares s_memtime (shader cycles) with s_memrealtime (the constant 100 MHz
 * wall clock) in every wave: *mhz = mean shader clock while the GPU was busy with it, *mhz_min / *mhz_max over the waves
 * (either may be NULL).  A kernel-time figure can then be read in cycles as well as in nanoseconds, and two runs on
 * two boxes compared by more than their wall clocks. */
int      wfahip_debug_clock(wfahip_ctx *ctx, double *mhz, double *mhz_min, double *mhz_max);
int      wfahip_generate_pairs_device(wfahip_ctx *ctx, uint64_t seed, uint64_t first_index, uint64_t n_pairs, uint32_t length,
                                      double error_rate, void *d_blob, void *d_q_off, void *d_q_len, void *d_t_off,
                                      void *d_t_len, void *stream);

#ifdef __cplusplus
}
#endif
#endif
