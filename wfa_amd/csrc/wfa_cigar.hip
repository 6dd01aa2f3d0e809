// wfa_cigar.hip -- CIGAR text rendered where the ops are (include/wfa_hip.h: wfahip_cigar_text_device, wfahip_cigar_text,
// wfahip_align_batch_text).  The rendering rule is wfa_cigar.hpp's, shared by the kernels and the host renderer.
//
// The alignment leaves a 64-byte record per pair and the pair's ops somewhere in the shared op buffer; a file writer wants
// AlignmentResult.CIGAR() of every pair.  That is the work wfa_finalize.hpp does for the result arrays once more -- a length per
// pair, a scan in pair order, a scatter -- with bytes in place of ops, and the ops are in HBM when it is needed:
//   wfa_cigar_len_kernel    a wave per pair, four pairs per block, lanes striding over the ops: the range that renders (under
//                           only_aligned the first to the last 'M' op, from ballots) and the bytes of its text (digits by compares)
//   the scan                exclusive, 64-bit, in pair order, in place in the caller's offset array: a block scan, the scan of the
//                           block sums, the bases added (wfa_cigar_scan_blocks / _sums / _add)
//   wfa_cigar_write_kernel  a wave per pair in rounds of 64 ops: each lane renders its own op, a wave prefix sum of the op lengths
//                           places it, the round's total is carried into the next round.  The bytes go straight to global memory.
//                           (A round staged in LDS and stored as aligned dwords measured 9 % slower: KERNELS.md 4p.)
// The host learns two numbers per call -- the total and whether a record points outside the op buffer -- from one 64-byte fetch.
//
// The display rows of AlignmentResult.AlignmentText (wfahip_alignment_text_device, wfahip_alignment_text; the rule is
// wfa_altext.hpp's) are the same three passes with the same scan kernels: wfa_altext_len_kernel adds the columns and the bases a
// pair's ops consume and checks them against the windows of its sequences, wfa_altext_write_kernel expands the runs -- a wave per
// pair in rounds of 64 ops, the round's table of starts in LDS, the lanes sweeping the round's columns four to a lane.
//
// The rows from 2-bit packed words, both strands (wfahip_alignment_text_packed_device, wfahip_alignment_text_packed; the decoding
// rule is wfa_altext_pk.hpp's): the same passes again, wfa_altext_pk_len_kernel with the window check on words and
// wfa_altext_pk_write_kernel, whose lanes take four letters out of two words by a funnel shift where the byte kernel loads four
// bytes, a flagged query's from the far end of its words, reversed and complemented (KERNELS.md 4t).
//
// The difference string (wfahip_diff_text_device, wfahip_diff_text_packed_device and their host entries; the rule is wfa_diff.hpp's):
// the rows' length pass with the bytes of the text as a fourth sum, the same scan, and wfa_diff_write_kernel /
// wfa_diff_pk_write_kernel -- a lane renders its own op where the token is short, the whole wave sweeps a long op (KERNELS.md 4v).
//
// The check (wfahip_check_alignments_device, wfahip_check_alignments_packed_device and their host entries; the rule is
// wfa_check.hpp's): ONE pass, wfa_check_kernel / wfa_check_pk_kernel, the write kernels' rounds and their column sweep (alt_sweep)
// with a sink that compares an M or X column's two bases where the write kernels store them; eight words and a status a pair,
// one counter to the host (KERNELS.md 4u).
//
// The pileup (wfahip_pileup_device, wfahip_pileup_packed_device and their host entries; the rule is wfa_pile.hpp's): the first product
// per TARGET BASE.  Two passes: the rows' length pass without its store and its scan, then wfa_pile_kernel / wfa_pile_pk_kernel -- the
// write kernels' rounds and table, the target-consuming columns swept by target base, one add without a return per column into
// the caller's eight counters a base (KERNELS.md 4w).
#include "wfa_ctx.hpp"
#include "wfa_hostpack.hpp"
#include "wfa_cigar.hpp"
#include "wfa_altext.hpp"
#include "wfa_altext_pk.hpp"
#include "wfa_check.hpp"
#include "wfa_diff.hpp"
#include "wfa_pile.hpp"

using namespace wfa;

namespace {

constexpr int CIG_SCAN_BLOCK = 1024, CIG_SCAN_ITEMS = 4;  // scan: pairs per block = CIG_SCAN_BLOCK * CIG_SCAN_ITEMS
constexpr uint64_t CIG_PER_BLOCK = (uint64_t)CIG_SCAN_BLOCK * CIG_SCAN_ITEMS;
constexpr int CIG_CTL_WORDS = 8;  // u64 counters, one 64-byte fetch: [0] total bytes [1] != 0: an OK record's ops leave the op buffer (the rows: or fail another check)
enum { CIG_TOTAL = 0, CIG_BAD_RANGE = 1 };
static_assert(CIG_CTL_WORDS * 8 <= HPIN_REDO * 4, "the counters fit the head of the pinned block");

struct CigParams {
    const uint32_t *rec;   // [n][REC_WORDS]
    const uint64_t *ops;   // the op buffer the records index
    uint64_t        ops_cap, n;
    uint32_t        only_aligned;
    uint64_t       *text_off;  // [n + 1]: lengths after the first pass, exclusive offsets (and the total) after the scan
    uint8_t        *text;
    uint64_t       *blk_sum;   // [n_blocks] bytes per scan block, then exclusive bases
    uint2          *range;     // [n] {first op that renders, number of ops that render}, relative to the pair's ops
    unsigned long long *ctl;   // [CIG_CTL_WORDS]
};

// the display rows: C's text_off is the rows' offset array (text is not used), CIG_BAD_RANGE is raised by every failed check
// (the difference string: the same struct with the text in C.text, the planes null and dwords saying that the TEXT is 4-byte aligned)
struct AltParams {
    CigParams       C;
    const uint8_t  *blob;
    uint64_t        blob_bytes;
    const uint64_t *q_off, *t_off;  // [n]
    const uint32_t *q_len, *t_len;  // [n]
    uint8_t        *q_row, *a_row, *t_row;
    uint32_t        dwords;  // != 0: the three planes are 4-byte aligned, four columns go out as one store
};

// the display rows from packed words: AltParams with the words in place of the blob, word offsets, and a flag per pair
struct AltPkParams {
    CigParams       C;
    const uint32_t *words;
    uint64_t        n_words;
    const uint64_t *q_woff, *t_woff;  // [n]
    const uint32_t *q_len, *t_len;    // [n]
    const uint8_t  *q_rc;             // [n] or null: != 0, the query is read reverse-complemented
    uint8_t        *q_row, *a_row, *t_row;
    uint32_t        dwords;
};

// the check (wfa_check.hpp): one struct for bytes and words -- seq is the blob or the words, seq_size blob_bytes or n_words, q_off /
// t_off byte or word offsets, q_rc only the words'
struct ChkParams {
    const uint32_t *rec;
    const uint64_t *ops;
    uint64_t        ops_cap, n;
    ChkRule         rule;
    uint32_t        mask;
    const void     *seq;
    uint64_t        seq_size;
    const uint64_t *q_off, *t_off;  // [n]
    const uint32_t *q_len, *t_len;  // [n]
    const uint8_t  *q_rc;           // [n] or null
    uint32_t       *chk;            // [n][CHK_WORDS]
    int32_t        *pass;           // [n] or null
    uint32_t        vec;            // != 0: chk is 16-byte aligned, a pair's words go out as two stores
    unsigned long long *ctl;        // [CIG_CTL_WORDS]: [CHK_FLAGGED] the OK pairs with a flag of the mask
};
enum { CHK_FLAGGED = 0 };
static_assert(CHK_WORDS == WFAHIP_CHK_WORDS && CHK_ALL == WFAHIP_CHK_ALL && CHK_PAIR_FAILED == WFAHIP_PAIR_CHECK_FAILED &&
                  CHK_OPS_RANGE == WFAHIP_CHK_OPS_RANGE && CHK_NO_M == WFAHIP_CHK_NO_M && CHK_SEQ_RANGE == WFAHIP_CHK_SEQ_RANGE &&
                  CHK_T_UNDER == WFAHIP_CHK_T_UNDER && CHK_X_EQUAL == WFAHIP_CHK_X_EQUAL && CHK_NO_ROWS_TRIMMED == WFAHIP_CHK_NO_ROWS_TRIMMED &&
                  CHK_COST_UNDER == WFAHIP_CHK_COST_UNDER && CHK_STAT_GAP_REGIONS == WFAHIP_CHK_STAT_GAP_REGIONS,
              "wfa_check.hpp's flags are the public header's");
constexpr uint32_t CHK_MAX_GRID = 2048;  // workgroups of four waves, each wave striding over the pairs
static_assert(PILE_WORDS == WFAHIP_PILE_WORDS && PILE_W_A == WFAHIP_PILE_W_A && PILE_W_C == WFAHIP_PILE_W_C && PILE_W_T == WFAHIP_PILE_W_T &&
                  PILE_W_G == WFAHIP_PILE_W_G && PILE_W_OTHER == WFAHIP_PILE_W_OTHER && PILE_W_GAP == WFAHIP_PILE_W_GAP &&
                  PILE_W_EXTRA == WFAHIP_PILE_W_EXTRA && PILE_W_EXTRA_BASES == WFAHIP_PILE_W_EXTRA_BASES,
              "wfa_pile.hpp's words are the public header's");

}  // namespace

// a wave's pair: the ops [*first, *end) of its *ops that render (under only_aligned the first to the last 'M' op, from ballots;
// none without one).  An OK record whose ops leave the op buffer raises CIG_BAD_RANGE and renders nothing.
__device__ __forceinline__ void cig_wave_range(const CigParams &C, uint64_t i, uint32_t lane, const uint64_t **ops_out, uint32_t *first_out,
                                               uint32_t *end_out) {
    const uint32_t *r   = C.rec + i * REC_WORDS;
    uint32_t        len = r[REC_STATUS] == ST_OK ? r[REC_OPS_LEN] : 0u;  // (fin_len's rule: a failed pair's record may hold stale words)
    const uint64_t  src = (uint64_t)r[REC_OPS_OFF_LO] | ((uint64_t)r[REC_OPS_OFF_HI] << 32);
    if (r[REC_STATUS] == ST_OK && (len > C.ops_cap || src > C.ops_cap - len)) {  // (compared without a sum that could wrap)
        if (lane == 0) atomicOr(&C.ctl[CIG_BAD_RANGE], 1ull);
        len = 0u;  // none of its ops is read
    }
    const uint64_t *ops = C.ops + (len != 0u ? src : 0ull);
    uint32_t first = 0u, end = len;  // the ops [first, end) render
    if (C.only_aligned != 0u) {
        first = len, end = 0u;
        for (uint32_t b = 0; b < len; b += 64u) {
            const uint32_t k = b + lane;
            const uint64_t m = __ballot(k < len && cig_is_m(ops[k]));
            if (m != 0ull) {
                if (first == len) first = b + (uint32_t)__builtin_ctzll(m);
                end = b + 64u - (uint32_t)__builtin_clzll(m);
            }
        }
        if (end == 0u) first = 0u;  // no 'M' op: nothing renders
    }
    *ops_out = ops, *first_out = first, *end_out = end;
}

// pass 1: the range of each pair's ops that renders and the bytes of its text
__global__ __launch_bounds__(256) void wfa_cigar_len_kernel(const CigParams C) {
    const uint64_t i    = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (i >= C.n) return;
    const uint64_t *ops;
    uint32_t        first, end;
    cig_wave_range(C, i, lane, &ops, &first, &end);
    unsigned long long bytes = 0ull;
    for (uint32_t k = first + lane; k < end; k += 64u) bytes += cig_op_bytes(ops[k]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bytes += __shfl_xor(bytes, o, 64);
    if (lane == 0) {
        C.text_off[i] = bytes;
        C.range[i]    = make_uint2(first, end - first);
    }
}

// pass 2a: exclusive offsets inside a block of CIG_PER_BLOCK pairs, in place, + the block's total (fin_scan_blocks' shape)
__global__ __launch_bounds__(CIG_SCAN_BLOCK) void wfa_cigar_scan_blocks(const CigParams C) {
    __shared__ unsigned long long wsum[CIG_SCAN_BLOCK / 64];
    const int      tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t i0  = ((uint64_t)blockIdx.x * CIG_SCAN_BLOCK + tid) * CIG_SCAN_ITEMS;
    unsigned long long v[CIG_SCAN_ITEMS], mine = 0ull;
#pragma unroll
    for (int k = 0; k < CIG_SCAN_ITEMS; k++) v[k] = i0 + k < C.n ? C.text_off[i0 + k] : 0ull, mine += v[k];
    unsigned long long incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    unsigned long long wbase = 0ull;
    for (int w = 0; w < wv; w++) wbase += wsum[w];
    unsigned long long run = wbase + incl - mine;
#pragma unroll
    for (int k = 0; k < CIG_SCAN_ITEMS; k++) {
        if (i0 + k < C.n) C.text_off[i0 + k] = run;
        run += v[k];
    }
    if (tid == CIG_SCAN_BLOCK - 1) C.blk_sum[blockIdx.x] = run;
}

// pass 2b: exclusive scan of the block sums (one block); the total lands in the counters and behind the last offset
__global__ __launch_bounds__(1024) void wfa_cigar_scan_sums(const CigParams C, uint32_t n_blocks) {
    __shared__ unsigned long long wsum[16];
    __shared__ unsigned long long carry;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) carry = 0ull;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += 1024) {
        const uint32_t     b    = b0 + tid;
        unsigned long long mine = b < n_blocks ? C.blk_sum[b] : 0ull, incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        unsigned long long wbase = carry;
        for (int w = 0; w < wv; w++) wbase += wsum[w];
        if (b < n_blocks) C.blk_sum[b] = wbase + incl - mine;
        __syncthreads();
        if (tid == 1023) carry = wbase + incl;
        __syncthreads();
    }
    if (tid == 0) C.ctl[CIG_TOTAL] = carry, C.text_off[C.n] = carry;
}

// pass 2c: the block bases added (block 0's is 0: its launch starts at the second scan block)
__global__ __launch_bounds__(256) void wfa_cigar_scan_add(const CigParams C) {
    const uint64_t i = CIG_PER_BLOCK + (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < C.n) C.text_off[i] += C.blk_sum[i / CIG_PER_BLOCK];
}

// pass 3: the text.  Lane l of round b renders op first + b + l at the pair's offset + the bytes of the ops before it.
__global__ __launch_bounds__(256) void wfa_cigar_write_kernel(const CigParams C) {
    const uint64_t i    = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (i >= C.n) return;
    const uint2 rg = C.range[i];
    if (rg.y == 0u) return;
    const uint32_t *r   = C.rec + i * REC_WORDS;
    const uint64_t *ops = C.ops + ((uint64_t)r[REC_OPS_OFF_LO] | ((uint64_t)r[REC_OPS_OFF_HI] << 32)) + rg.x;
    uint8_t        *dst = C.text + C.text_off[i];  // (the carry between rounds moves it on)
    for (uint32_t b = 0; b < rg.y; b += 64u) {
        const uint32_t k    = b + lane;
        const bool     have = k < rg.y;
        const uint64_t op   = have ? ops[k] : 0ull;
        const uint32_t mine = have ? cig_op_bytes(op) : 0u;
        uint32_t       incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(incl, o, 64);
            if (lane >= (uint32_t)o) incl += t;
        }
        if (have) cig_render(op, dst + (incl - mine));
        dst += __shfl(incl, 63, 64);  // (at most 64 x 11 bytes a round)
    }
}

// ---- the display rows (wfa_altext.hpp)

// the windows of pair i's sequences, from its record and the caller's four arrays
__device__ __forceinline__ bool alt_pair_window(const AltParams &A, uint64_t i, AltWindow *w) {
    const uint32_t *r = A.C.rec + i * REC_WORDS;
    return alt_window(A.C.only_aligned != 0u, A.blob_bytes, A.q_off[i], A.q_len[i], A.t_off[i], A.t_len[i], (int32_t)r[REC_QBEGIN],
                      (int32_t)r[REC_QEND], (int32_t)r[REC_TBEGIN], (int32_t)r[REC_TEND], w);
}

__device__ __forceinline__ uint32_t alt_load4(const uint8_t *p) {  // four bytes at any alignment
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// rows, pass 1: the range of each pair's ops that renders, its columns, and every check that keeps pass 3 inside the op buffer,
// the sequences and the windows -- window(i, &w) gives pair i's windows, false where they fail.  A pair that fails a check raises
// CIG_BAD_RANGE; pass 3 is then not launched.  The byte entry checks the windows of every pair with an op in its range; the packed
// entry (COLUMNS_ONLY) only those of a pair with a column, so that the offsets of a pair that renders nothing are never looked at.
// DIFF: the pass of the difference string (wfa_diff.hpp) -- the same checks, and a fourth sum, the bytes of the text, is what
// text_off[i] receives in place of the columns (a pair has a byte exactly when it has a column).
// PILE: the pass of the pileup (wfa_pile.hpp) -- the same checks again; no offset is stored (nothing is scanned), and lane 0 returns
// whether the pair has a column, which is all the entry counts.
template <bool COLUMNS_ONLY, bool DIFF = false, bool PILE = false, class Window>
__device__ __forceinline__ bool alt_len_pair(const CigParams &C, uint64_t i, uint32_t lane, Window &&window) {
    const uint64_t *ops;
    uint32_t        first, end;
    cig_wave_range(C, i, lane, &ops, &first, &end);
    AltSums            s     = {0, 0, 0};
    unsigned long long bytes = 0ull;  // (DIFF only)
    for (uint32_t k = first + lane; k < end; k += 64u) {
        alt_add(&s, ops[k]);
        if constexpr (DIFF) bytes += diff_op_bytes(ops[k]);
    }
    unsigned long long cols = s.cols, qb = s.q, tb = s.t;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cols += __shfl_xor(cols, o, 64);
        qb += __shfl_xor(qb, o, 64);
        tb += __shfl_xor(tb, o, 64);
        if constexpr (DIFF) bytes += __shfl_xor(bytes, o, 64);
    }
    if (lane == 0) {
        uint32_t count = end - first;
        if (COLUMNS_ONLY ? cols != 0ull : count != 0u) {
            const AltSums all = {cols, qb, tb};
            AltWindow     w;
            if (!window(i, &w) || !alt_fits(all, w)) {
                atomicOr(&C.ctl[CIG_BAD_RANGE], 1ull);
                cols = 0ull;
            }
        }
        if (cols == 0ull) count = 0u;  // (ops without a column: pass 3 has nothing to do)
        if constexpr (!PILE) C.text_off[i] = DIFF ? (cols != 0ull ? bytes : 0ull) : cols;
        C.range[i] = make_uint2(first, count);
    }
    return cols != 0ull;
}

template <bool COLUMNS_ONLY, bool DIFF = false, class Window>
__device__ __forceinline__ void alt_len_pass(const CigParams &C, Window &&window) {
    const uint64_t i    = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (i >= C.n) return;
    (void)alt_len_pair<COLUMNS_ONLY, DIFF>(C, i, lane, window);
}

__global__ __launch_bounds__(256) void wfa_altext_len_kernel(const AltParams A) {
    alt_len_pass<false>(A.C, [&](uint64_t i, AltWindow *w) { return alt_pair_window(A, i, w); });
}

// the windows of pair i's packed sequences, in bases of each sequence (the offsets of a pair that renders nothing are not looked at:
// only a pair with an op that renders gets here)
__device__ __forceinline__ bool alt_pk_pair_window(const AltPkParams &A, uint64_t i, AltWindow *w) {
    const uint32_t *r = A.C.rec + i * REC_WORDS;
    return alt_pk_window(A.C.only_aligned != 0u, A.n_words, A.q_woff[i], A.q_len[i], A.t_woff[i], A.t_len[i], (int32_t)r[REC_QBEGIN],
                         (int32_t)r[REC_QEND], (int32_t)r[REC_TBEGIN], (int32_t)r[REC_TEND], w);
}

__global__ __launch_bounds__(256) void wfa_altext_pk_len_kernel(const AltPkParams A) {
    alt_len_pass<true>(A.C, [&](uint64_t i, AltWindow *w) { return alt_pk_pair_window(A, i, w); });
}

// rows, pass 3.  A round is 64 ops: a wave prefix sum gives every op its first column of the round and its first query and target
// byte of the windows, and the table goes to the wave's LDS.  The lanes then sweep the round's columns in groups of four that are
// aligned in the PLANE (not in the pair), consecutive lanes taking consecutive groups: a lane finds the op of its first column by a
// search over the 64 starts and walks on from there.  A group inside one op -- most of them -- is one 4-byte load per sequence
// and, where the planes are 4-byte aligned, one 4-byte store per plane; a group that crosses an op boundary gathers byte by byte;
// a group cut by the round's first or last column stores bytes, and the next round stores the rest of it.
// Where the bases come from is the kernel's: seq(i) gives pair i's source once pass 1 has found it valid, with q4(p) / t4(p) the
// four query / target bases from base p of the window on (base p + j in bits 8 j ..) and q1(p) / t1(p) one base.
// The sweep of a round's columns [g0, gend) of at most R (the check kernels stop at the last column they compare): tab_* is the
// wave's table of the round, sink(g, j0, j1, qv, av, tv) takes the columns g + j0 .. g + j1 - 1 of the group at g, column g + j in
// bits 8 j .. of the three words.  ONE copy for the kernels that write rows and the ones that check them.
template <class Seq, class Sink>
__device__ __forceinline__ void alt_sweep(const unsigned long long *tab_col, const uint32_t *tab_q, const uint32_t *tab_t, const uint32_t *tab_kind,
                                          uint32_t lane, uint64_t g0, uint64_t gend, unsigned long long R, const Seq &S, Sink &&sink) {
    for (uint64_t g = (g0 & ~3ull) + 4u * lane; g < gend; g += 256u) {
        const uint64_t lo = g > g0 ? g : g0, hi = g + 4u < gend ? g + 4u : gend;  // the group's columns of this round: lo < hi
        const uint32_t j0 = (uint32_t)(lo - g), j1 = (uint32_t)(hi - g);
        unsigned long long c = lo - g0;  // column in the round, < R
        uint32_t           k = 0u;       // the last op whose first column is <= c: the one with a column there
#pragma unroll
        for (uint32_t step = 32u; step != 0u; step >>= 1)
            if (tab_col[k + step] <= c) k += step;
        unsigned long long cs = tab_col[k], ce = k < 63u ? tab_col[k + 1u] : R;
        uint32_t           kd = tab_kind[k], qb = tab_q[k], tb = tab_t[k];
        uint32_t           qv = 0u, av = 0u, tv = 0u;  // the group's bytes, column g + j in bits 8 j ..
        if (j1 - j0 == 4u && c + 4u <= ce) {
            const uint64_t d = c - cs;
            qv = (kd & ALT_Q) ? S.q4((uint64_t)qb + d) : ALT_GAP * 0x01010101u;
            tv = (kd & ALT_T) ? S.t4((uint64_t)tb + d) : ALT_GAP * 0x01010101u;
            av = (kd >> 8) * 0x01010101u;
        } else {
            for (uint32_t j = j0; j < j1; j++, c++) {
                if (c >= ce) {
                    do {  // (ops without a column have cs == ce; c < R ends the walk at op 63 at the latest)
                        k++;
                        cs = ce, ce = k < 63u ? tab_col[k + 1u] : R;
                    } while (c >= ce);
                    kd = tab_kind[k], qb = tab_q[k], tb = tab_t[k];
                }
                const uint64_t d  = c - cs;
                const uint32_t qx = (kd & ALT_Q) ? S.q1((uint64_t)qb + d) : ALT_GAP, tx = (kd & ALT_T) ? S.t1((uint64_t)tb + d) : ALT_GAP;
                qv |= qx << (8u * j), av |= (kd >> 8) << (8u * j), tv |= tx << (8u * j);
            }
        }
        sink(g, j0, j1, qv, av, tv);
    }
}

template <class Params, class Seq>
__device__ __forceinline__ void alt_write_pass(const Params &A, Seq &&seq) {
    __shared__ unsigned long long s_col[4][64];                      // first column of the op, in the round
    __shared__ uint32_t           s_q[4][64], s_t[4][64], s_kind[4][64];  // first query / target byte in the windows; alt_kind | a byte << 8
    const CigParams &C    = A.C;
    const uint32_t   wv   = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t   i    = (uint64_t)blockIdx.x * 4 + wv;
    if (i >= C.n) return;
    const uint2 rg = C.range[i];
    if (rg.y == 0u) return;
    const auto      S   = seq(i);
    const uint32_t *r   = C.rec + i * REC_WORDS;
    const uint64_t *ops = C.ops + ((uint64_t)r[REC_OPS_OFF_LO] | ((uint64_t)r[REC_OPS_OFF_HI] << 32)) + rg.x;
    uint64_t        g0 = C.text_off[i];  // the round's first column, as an index into the planes
    uint32_t        qc = 0u, tc = 0u;    // bases the rounds before consumed (pass 1: at most the windows' lengths)
    for (uint32_t b = 0; b < rg.y; b += 64u) {
        const uint64_t     op   = b + lane < rg.y ? ops[b + lane] : 0ull;  // (letter 0: no column)
        const uint32_t     kind = alt_kind(op), cnt = alt_cols(op);
        const uint32_t     myq = (kind & ALT_Q) ? cnt : 0u, myt = (kind & ALT_T) ? cnt : 0u;
        unsigned long long ci = cnt;  // (64 counts of a full u32 each)
        uint32_t           qi = myq, ti = myt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long c2 = __shfl_up(ci, o, 64);
            const uint32_t           q2 = __shfl_up(qi, o, 64), t2 = __shfl_up(ti, o, 64);
            if (lane >= (uint32_t)o) ci += c2, qi += q2, ti += t2;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (the round before has read its table)
        __builtin_amdgcn_wave_barrier();
        s_col[wv][lane]  = ci - cnt;
        s_q[wv][lane]    = qc + qi - myq;
        s_t[wv][lane]    = tc + ti - myt;
        s_kind[wv][lane] = kind | ((uint32_t)alt_a_byte(op) << 8);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const unsigned long long R    = __shfl(ci, 63, 64);  // the round's columns
        const uint64_t           gend = g0 + R;
        alt_sweep(s_col[wv], s_q[wv], s_t[wv], s_kind[wv], lane, g0, gend, R, S,
                  [&](uint64_t g, uint32_t j0, uint32_t j1, uint32_t qv, uint32_t av, uint32_t tv) {
                      if (j1 - j0 == 4u && A.dwords != 0u) {
                          *reinterpret_cast<uint32_t *>(A.q_row + g) = qv;
                          *reinterpret_cast<uint32_t *>(A.a_row + g) = av;
                          *reinterpret_cast<uint32_t *>(A.t_row + g) = tv;
                      } else {
                          for (uint32_t j = j0; j < j1; j++) {
                              A.q_row[g + j] = (uint8_t)(qv >> (8u * j));
                              A.a_row[g + j] = (uint8_t)(av >> (8u * j));
                              A.t_row[g + j] = (uint8_t)(tv >> (8u * j));
                          }
                      }
                  });
        g0 = gend;
        qc += __shfl(qi, 63, 64), tc += __shfl(ti, 63, 64);
    }
}

// the windows' first bytes in the blob
struct AltByteSeq {
    const uint8_t *qs, *ts;
    __device__ __forceinline__ uint32_t q4(uint64_t p) const { return alt_load4(qs + p); }
    __device__ __forceinline__ uint32_t t4(uint64_t p) const { return alt_load4(ts + p); }
    __device__ __forceinline__ uint32_t q1(uint64_t p) const { return qs[p]; }
    __device__ __forceinline__ uint32_t t1(uint64_t p) const { return ts[p]; }
};

__global__ __launch_bounds__(256) void wfa_altext_write_kernel(const AltParams A) {
    alt_write_pass(A, [&](uint64_t i) {
        AltWindow w;
        (void)alt_pair_window(A, i, &w);  // (pass 1 found it valid, and the ops inside it)
        return AltByteSeq{A.blob + w.q_at, A.blob + w.t_at};
    });
}

// the sequences' words and the windows' first bases.  Base p of a window is base at + p of the sequence (pass 1: at + p < len, so
// the sums stay below 2^32); a group of four inside one op lies inside the window, which is what alt_pk_letters4 asks for.
struct AltPkSeq {
    const uint32_t *qw, *tw;
    uint32_t        q_len, t_len, q_at, t_at;
    bool            rc;  // (one pair a wave: uniform)
    __device__ __forceinline__ uint32_t q4(uint64_t p) const { return alt_pk_letters4(qw, q_len, rc, q_at + (uint32_t)p); }
    __device__ __forceinline__ uint32_t t4(uint64_t p) const { return alt_pk_letters4(tw, t_len, false, t_at + (uint32_t)p); }
    __device__ __forceinline__ uint32_t q1(uint64_t p) const { return alt_pk_letter(qw, q_len, rc, q_at + (uint32_t)p); }
    __device__ __forceinline__ uint32_t t1(uint64_t p) const { return alt_pk_letter(tw, t_len, false, t_at + (uint32_t)p); }
};

// rows from packed words, pass 3: wfa_altext_write_kernel's rounds, groups and stores.  A group inside one op is a funnel shift over
// two words per sequence and one v_perm_b32 from codes to letters; a flagged query reads the four bases that END at len - 1 - p.
__global__ __launch_bounds__(256) void wfa_altext_pk_write_kernel(const AltPkParams A) {
    alt_write_pass(A, [&](uint64_t i) {
        AltWindow w;
        (void)alt_pk_pair_window(A, i, &w);  // (pass 1 found it valid, and the ops inside it)
        return AltPkSeq{A.words + A.q_woff[i], A.words + A.t_woff[i], A.q_len[i], A.t_len[i], (uint32_t)w.q_at, (uint32_t)w.t_at,
                        A.q_rc != nullptr && A.q_rc[i] != 0};
    });
}

// ---- the difference string (wfa_diff.hpp)

__global__ __launch_bounds__(256) void wfa_diff_len_kernel(const AltParams A) {
    alt_len_pass<false, true>(A.C, [&](uint64_t i, AltWindow *w) { return alt_pair_window(A, i, w); });
}

__global__ __launch_bounds__(256) void wfa_diff_pk_len_kernel(const AltPkParams A) {
    alt_len_pass<true, true>(A.C, [&](uint64_t i, AltWindow *w) { return alt_pk_pair_window(A, i, w); });
}

// the string, pass 3.  A round is 64 ops, a lane an op: wave prefix sums give every op its first byte of the text (64-bit: one 'X' op
// may render 3 x 0xFFFFFFFF bytes) and its first query and target base of the windows.  Typical ops are short -- at 5 % error nearly
// every token has 3 to 6 bytes -- so a lane renders its own op where the text has at most DIFF_LANE_BYTES bytes (diff_render, the
// host's function: an 'M' op always, an 'X' op of up to 5 columns, a gap of up to 15 letters), as wfa_cigar_write_kernel does.  The
// longer ops are found by a ballot and the WHOLE wave sweeps each in turn, four bytes to a lane in groups that are aligned in the
// text buffer: no lane walks a count.  A group inside a gap's letters is one q4 / t4 and one store where d_text is 4-byte aligned;
// an 'X' op's group, and one cut by the op's first or last byte, gathers byte by byte (diff_op_byte).  The op a sweep works on is
// uniform, so its start, length and bases come by __shfl from the lane that holds it: the round needs no table in LDS, and no fence.
// An 'M' op loads no sequence byte, a gap only its own side's.
template <class Params, class MakeSeq>
__device__ __forceinline__ void diff_write_pass(const Params &A, MakeSeq &&seq) {
    const CigParams &C    = A.C;
    const uint32_t   lane = threadIdx.x & 63;
    const uint64_t   i    = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= C.n) return;
    const uint2 rg = C.range[i];
    if (rg.y == 0u) return;
    const auto         S   = seq(i);
    const uint32_t    *r   = C.rec + i * REC_WORDS;
    const uint64_t    *ops = C.ops + ((uint64_t)r[REC_OPS_OFF_LO] | ((uint64_t)r[REC_OPS_OFF_HI] << 32)) + rg.x;
    unsigned long long at  = C.text_off[i];  // the round's first byte, as an index into the text
    uint32_t           qc = 0u, tc = 0u;     // bases the rounds before consumed (pass 1: at most the windows' lengths)
    for (uint32_t b = 0; b < rg.y; b += 64u) {
        const uint64_t           op   = b + lane < rg.y ? ops[b + lane] : 0ull;  // (letter 0: no byte)
        const uint32_t           kind = alt_kind(op), cnt = alt_cols(op);
        const uint32_t           myq = (kind & ALT_Q) ? cnt : 0u, myt = (kind & ALT_T) ? cnt : 0u;
        const unsigned long long mine = diff_op_bytes(op);
        unsigned long long       bi = mine;
        uint32_t                 qi = myq, ti = myt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long b2 = __shfl_up(bi, o, 64);
            const uint32_t           q2 = __shfl_up(qi, o, 64), t2 = __shfl_up(ti, o, 64);
            if (lane >= (uint32_t)o) bi += b2, qi += q2, ti += t2;
        }
        const unsigned long long start = at + bi - mine;
        const uint32_t           qp = qc + qi - myq, tp = tc + ti - myt;
        if (mine != 0ull && mine <= DIFF_LANE_BYTES) diff_render(op, S, qp, tp, C.text + start);
        for (uint64_t big = __ballot(mine > DIFF_LANE_BYTES); big != 0ull; big &= big - 1ull) {  // (an 'X' op or a gap: diff_op_byte's)
            const int                l  = __builtin_ctzll(big);
            const unsigned long long a  = __shfl(start, l, 64), e = a + __shfl(mine, l, 64);
            const uint32_t           kd = __shfl(kind, l, 64), oq = __shfl(qp, l, 64), ot = __shfl(tp, l, 64);
            for (unsigned long long g = (a & ~3ull) + 4u * lane; g < e; g += 256u) {
                const unsigned long long lo = g > a ? g : a, hi = g + 4u < e ? g + 4u : e;  // the group's bytes of this op: lo < hi
                const unsigned long long x  = lo - a;                                       // the first one's place in the op's text
                const uint32_t           nb = (uint32_t)(hi - lo);
                uint32_t                 v  = 0u;  // byte lo + j in bits 8 j ..
                if (nb == 4u && kd != (ALT_Q | ALT_T) && x != 0ull) {
                    v = diff_lc4(kd == ALT_T ? S.t4(ot + x - 1u) : S.q4(oq + x - 1u));
                } else {
                    for (uint32_t j = 0; j < nb; j++) v |= diff_op_byte(kd, S, oq, ot, x + j) << (8u * j);
                }
                if (nb == 4u && A.dwords != 0u) {
                    *reinterpret_cast<uint32_t *>(C.text + g) = v;  // (lo == g)
                } else {
                    for (uint32_t j = 0; j < nb; j++) C.text[lo + j] = (uint8_t)(v >> (8u * j));
                }
            }
        }
        at += __shfl(bi, 63, 64);
        qc += __shfl(qi, 63, 64), tc += __shfl(ti, 63, 64);
    }
}

__global__ __launch_bounds__(256) void wfa_diff_write_kernel(const AltParams A) {
    diff_write_pass(A, [&](uint64_t i) {
        AltWindow w;
        (void)alt_pair_window(A, i, &w);  // (pass 1 found it valid, and the ops inside it)
        return AltByteSeq{A.blob + w.q_at, A.blob + w.t_at};
    });
}

__global__ __launch_bounds__(256) void wfa_diff_pk_write_kernel(const AltPkParams A) {
    diff_write_pass(A, [&](uint64_t i) {
        AltWindow w;
        (void)alt_pk_pair_window(A, i, &w);  // (pass 1 found it valid, and the ops inside it)
        return AltPkSeq{A.words + A.q_woff[i], A.words + A.t_woff[i], A.q_len[i], A.t_len[i], (uint32_t)w.q_at, (uint32_t)w.t_at,
                        A.q_rc != nullptr && A.q_rc[i] != 0};
    });
}

// ---- the pileup (wfa_pile.hpp)

// pileup, pass 1: the rows' length pass (alt_len_pair) with the waves striding over the pairs, so that ONE atomic a wave feeds the
// count of the pairs that pass 2 sweeps
template <bool COLUMNS_ONLY, class Window>
__device__ __forceinline__ void pile_len_pass(const CigParams &C, Window &&window) {
    const uint32_t lane  = threadIdx.x & 63;
    uint32_t       piled = 0u;  // (lane 0's)
    for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < C.n; i += (uint64_t)gridDim.x * 4)
        piled += alt_len_pair<COLUMNS_ONLY, false, true>(C, i, lane, window) ? 1u : 0u;
    if (lane == 0 && piled != 0u) atomicAdd(&C.ctl[CIG_TOTAL], (unsigned long long)piled);
}

__global__ __launch_bounds__(256) void wfa_pile_len_kernel(const AltParams A) {
    pile_len_pass<false>(A.C, [&](uint64_t i, AltWindow *w) { return alt_pair_window(A, i, w); });
}

__global__ __launch_bounds__(256) void wfa_pile_pk_len_kernel(const AltPkParams A) {
    pile_len_pass<true>(A.C, [&](uint64_t i, AltWindow *w) { return alt_pk_pair_window(A, i, w); });
}

// one counter up by v: relaxed, device scope, the result unused -- an add without a return, nothing to wait for
__device__ __forceinline__ void pile_add(uint32_t *counts, uint64_t idx, uint32_t word, uint32_t v) {
    (void)__hip_atomic_fetch_add(counts + idx * PILE_WORDS + word, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// pileup, pass 2.  A wave per pair in rounds of 64 ops, a lane an op: wave prefix sums give every op its first query and target base
// of the windows, and the table goes to the wave's LDS as in alt_write_pass.  A 'D' op's two adds are its own lane's.  The columns
// that consume a target base ('M', 'X', 'I') are swept by TARGET BASE, not by op: each of them maps to exactly one base, the round's
// bases are one run [tc, tc + R), and only the part of it inside the pileup's window is walked (pile_clip) -- consecutive lanes take
// consecutive bases, so that one wave add falls into 64 x 32 B = 2 KB of the counters, and a lane finds the op of its base by a
// search over the table's 64 target starts (the last op that starts at or before the base is the one that consumes it: an op
// without a target base starts where the next one does).  No lane walks a count, and a window that misses the pair costs it one
// round of prefix sums per 64 ops and no memory access but its ops.  seq(i, &T0, &t_n) gives pair i's query reader, the coordinate
// of its target window's first base and that window's length, once pass 1 has found the pair valid.
template <class Params, class MakeSeq>
__device__ __forceinline__ void pile_pass(const Params &A, const PileWin W, uint32_t *counts, MakeSeq &&seq) {
    __shared__ uint32_t s_q[4][64], s_t[4][64], s_gap[4][64];  // first query / target base in the windows; != 0: the op is an 'I'
    const CigParams &C    = A.C;
    const uint32_t   wv   = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t   i    = (uint64_t)blockIdx.x * 4 + wv;
    if (i >= C.n) return;
    const uint2 rg = C.range[i];
    if (rg.y == 0u) return;
    uint64_t        T0;
    uint32_t        t_n;
    const auto      S   = seq(i, &T0, &t_n);
    const uint32_t *r   = C.rec + i * REC_WORDS;
    const uint64_t *ops = C.ops + ((uint64_t)r[REC_OPS_OFF_LO] | ((uint64_t)r[REC_OPS_OFF_HI] << 32)) + rg.x;
    uint32_t        qc = 0u, tc = 0u;  // bases the rounds before consumed (pass 1: at most the windows' lengths)
    for (uint32_t b = 0; b < rg.y; b += 64u) {
        const uint64_t op   = b + lane < rg.y ? ops[b + lane] : 0ull;  // (letter 0: no column)
        const uint32_t kind = alt_kind(op), cnt = alt_cols(op);
        const uint32_t myq = (kind & ALT_Q) ? cnt : 0u, myt = (kind & ALT_T) ? cnt : 0u;
        uint32_t       qi = myq, ti = myt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t q2 = __shfl_up(qi, o, 64), t2 = __shfl_up(ti, o, 64);
            if (lane >= (uint32_t)o) qi += q2, ti += t2;
        }
        const uint32_t qs = qc + qi - myq, ts = tc + ti - myt;  // the op's first bases
        if ((uint32_t)(op >> 32) == (uint32_t)'D' && cnt != 0u && t_n != 0u) {
            uint64_t idx;
            if (pile_in(pile_extra_base(T0, ts), W, &idx)) {
                pile_add(counts, idx, PILE_W_EXTRA, 1u);
                pile_add(counts, idx, PILE_W_EXTRA_BASES, cnt);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (the round before has read its table)
        __builtin_amdgcn_wave_barrier();
        s_q[wv][lane]   = qs;
        s_t[wv][lane]   = ts;
        s_gap[wv][lane] = kind == ALT_T ? 1u : 0u;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const uint32_t R = __shfl(ti, 63, 64);  // the round's target bases: [tc, tc + R) of the window
        uint64_t       lo, hi;
        if (pile_clip(T0 + tc, R, W, &lo, &hi)) {
            const uint64_t idx0 = T0 + tc - W.at;  // (mod 2^64; idx0 + x is the place of the round's base x wherever lo <= x < hi)
            for (uint64_t x = lo + lane; x < hi; x += 64u) {
                const uint32_t tb = tc + (uint32_t)x;
                uint32_t       k  = 0u;  // the last op whose first target base is <= tb: the one that consumes it
#pragma unroll
                for (uint32_t step = 32u; step != 0u; step >>= 1)
                    if (s_t[wv][k + step] <= tb) k += step;
                const uint32_t word = s_gap[wv][k] != 0u ? (uint32_t)PILE_W_GAP : S.word((uint64_t)s_q[wv][k] + (tb - s_t[wv][k]));
                pile_add(counts, idx0 + x, word, 1u);
            }
        }
        qc += __shfl(qi, 63, 64), tc += R;
    }
}

__global__ __launch_bounds__(256) void wfa_pile_kernel(const AltParams A, const PileWin W, uint32_t *counts) {
    pile_pass(A, W, counts, [&](uint64_t i, uint64_t *T0, uint32_t *t_n) {
        AltWindow w;
        (void)alt_pair_window(A, i, &w);  // (pass 1 found it valid, and the ops inside it)
        *T0 = w.t_at, *t_n = w.t_n;
        return PileByteSeq{A.blob + w.q_at};
    });
}

// the codes come straight from the words: no letter is made
__global__ __launch_bounds__(256) void wfa_pile_pk_kernel(const AltPkParams A, const PileWin W, uint32_t *counts) {
    pile_pass(A, W, counts, [&](uint64_t i, uint64_t *T0, uint32_t *t_n) {
        AltWindow w;
        (void)alt_pk_pair_window(A, i, &w);  // (pass 1 found it valid, and the ops inside it)
        *T0 = 16ull * A.t_woff[i] + w.t_at, *t_n = w.t_n;
        return PilePkSeq{A.words + A.q_woff[i], A.q_len[i], (uint32_t)w.q_at, A.q_rc != nullptr && A.q_rc[i] != 0};
    });
}

// ---- the check (wfa_check.hpp)

// A wave per pair, the waves striding over the pairs so that ONE atomic a wave feeds the counter.  The ops are read twice: ballots
// over cig_is_m give the first and the last 'M' op (the ranges step 8 and step 10 sum over), then rounds of 64 ops as in
// alt_write_pass -- a lane an op, step 3's flags from the op and its left neighbour (the round before hands its last letter on),
// the 64-bit wave prefix sums of columns, query and target bases, the table in LDS -- and alt_sweep over the round's columns up to
// the last one that step 7 compares.  The table names only 'M' and 'X' ops as reading bases (a byte of 1 / 2), so a gap's columns
// cost a lane no load and no base outside a sequence is touched; the sink compares where the row kernels store.  Nothing
// variable-length is written: no scan.  Lane 0 ends in chk_finish, the same as the host's chk_pair.
template <bool PACKED, class MakeSeq>
__device__ __forceinline__ void chk_wave_pass(const ChkParams &K, MakeSeq &&make_seq) {
    __shared__ unsigned long long s_col[4][64];
    __shared__ uint32_t           s_q[4][64], s_t[4][64], s_kind[4][64];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t       flagged = 0u;  // (lane 0's)
    for (uint64_t i = (uint64_t)blockIdx.x * 4 + wv; i < K.n; i += (uint64_t)gridDim.x * 4) {
        const uint32_t *r      = K.rec + i * REC_WORDS;
        const uint32_t  status = r[REC_STATUS];
        uint32_t        out[CHK_WORDS];
        if (status != ST_OK) {
            chk_unread(false, out);  // (a failed pair's record may hold stale words: none is read)
        } else {
            const uint32_t len = r[REC_OPS_LEN];
            const uint64_t src = (uint64_t)r[REC_OPS_OFF_LO] | ((uint64_t)r[REC_OPS_OFF_HI] << 32);
            if (chk_ops_range(src, len, K.ops_cap)) {
                chk_unread(true, out);
            } else {
                const uint64_t *ops   = K.ops + (len != 0u ? src : 0ull);
                const uint32_t  q_len = K.q_len[i], t_len = K.t_len[i];
                const auto      window = [&](bool trim, AltWindow *w) {
                    const int32_t qb = (int32_t)r[REC_QBEGIN], qe = (int32_t)r[REC_QEND], tb = (int32_t)r[REC_TBEGIN], te = (int32_t)r[REC_TEND];
                    return PACKED ? alt_pk_window(trim, K.seq_size, K.q_off[i], q_len, K.t_off[i], t_len, qb, qe, tb, te, w)
                                  : alt_window(trim, K.seq_size, K.q_off[i], q_len, K.t_off[i], t_len, qb, qe, tb, te, w);
                };
                // cig_range(ops, len, true, ..) from ballots
                uint32_t m_first = 0u, m_end = 0u;
                for (uint32_t b = 0; b < len; b += 64u) {
                    const uint64_t m = __ballot(b + lane < len && cig_is_m(ops[b + lane]));
                    if (m != 0ull) {
                        if (m_end == 0u) m_first = b + (uint32_t)__builtin_ctzll(m);
                        m_end = b + 64u - (uint32_t)__builtin_clzll(m);
                    }
                }
                ChkTotals T = {};
                T.len       = len;
                T.m_count   = m_end != 0u ? m_end - m_first : 0u;
                uint32_t s_first, s_count;
                chk_stat_range(len, m_first, T.m_count, &s_first, &s_count);
                AltWindow  w0;
                const bool seq_ok = window(false, &w0);
                const auto S      = make_seq(i, q_len, t_len);  // (nothing is read through it unless seq_ok)
                uint32_t   fl = (T.m_count == 0u ? CHK_NO_M : 0u) | (seq_ok ? 0u : CHK_SEQ_RANGE);
                uint64_t   cost = 0ull, n_bad = 0ull, first_bad = ~0ull;
                uint64_t   g0 = 0ull, qc = 0ull, tc = 0ull;  // columns and bases of the rounds before
                uint32_t   prev_last = 0u;                   // the last letter of the round before
                for (uint32_t b = 0; b < len; b += 64u) {
                    const uint32_t k      = b + lane;
                    const bool     have   = k < len;
                    const uint64_t op     = have ? ops[k] : 0ull;  // (letter 0: no column)
                    const uint32_t letter = (uint32_t)(op >> 32);
                    const uint32_t left   = __shfl_up(letter, 1, 64);
                    if (have) {
                        fl |= chk_op_flags(op, k != 0u, lane != 0u ? left : prev_last);
                        cost = chk_sat_add(cost, chk_op_cost(op, K.rule));
                        if (k - s_first < s_count) chk_stat_add(&T.stats, op);
                        if (k - m_first < T.m_count) alt_add(&T.trimmed, op);
                    }
                    const uint32_t     kind = alt_kind(op), cnt = alt_cols(op);
                    const uint64_t     myq = (kind & ALT_Q) ? cnt : 0u, myt = (kind & ALT_T) ? cnt : 0u;
                    unsigned long long ci = cnt, qi = myq, ti = myt;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const unsigned long long c2 = __shfl_up(ci, o, 64), q2 = __shfl_up(qi, o, 64), t2 = __shfl_up(ti, o, 64);
                        if (lane >= (uint32_t)o) ci += c2, qi += q2, ti += t2;
                    }
                    const uint64_t qs = qc + qi - myq, ts = tc + ti - myt;  // the op's first bases, true sums
                    const bool     cmp = chk_compares(op);
                    const uint32_t v   = seq_ok && cmp ? chk_valid(cnt, qs, ts, q_len, t_len) : 0u;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (the round before has read its table)
                    __builtin_amdgcn_wave_barrier();
                    s_col[wv][lane]  = ci - cnt;
                    s_q[wv][lane]    = (uint32_t)qs;  // (below q_len wherever a column of the op is compared)
                    s_t[wv][lane]    = (uint32_t)ts;
                    s_kind[wv][lane] = cmp ? (ALT_Q | ALT_T) | ((cig_is_m(op) ? 1u : 2u) << 8) : 0u;
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    const unsigned long long R  = __shfl(ci, 63, 64);  // the round's columns
                    const uint64_t           vm = __ballot(v != 0u);
                    if (vm != 0ull) {
                        // the compared columns are a prefix of the 'M' / 'X' columns: they end in the last op that has one
                        const unsigned long long E = __shfl(ci - cnt + v, 63 - __builtin_clzll(vm), 64);
                        alt_sweep(s_col[wv], s_q[wv], s_t[wv], s_kind[wv], lane, g0, g0 + E, R, S,
                                  [&](uint64_t g, uint32_t j0, uint32_t j1, uint32_t qv, uint32_t av, uint32_t tv) {
                                      // bit 7 of byte j: the bytes of column g + j differ; an M column (byte 1) is bad if they do,
                                      // an X column (byte 2) if they do not; the columns j0 .. j1 - 1 count
                                      const uint32_t x   = qv ^ tv;
                                      const uint32_t nz  = (x | ((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu)) & 0x80808080u;
                                      const uint32_t in  = (0xFFFFFFFFu >> (8u * (4u - j1))) & (0xFFFFFFFFu << (8u * j0));
                                      const uint32_t bad = ((nz & (av << 7)) | (~nz & (av << 6))) & 0x80808080u & in;
                                      if (bad != 0u) {  // (rare)
                                          if ((bad & nz) != 0u) fl |= CHK_M_DIFFERS;
                                          if ((bad & ~nz) != 0u) fl |= CHK_X_EQUAL;
                                          n_bad += (uint32_t)__builtin_popcount(bad);
                                          const uint64_t at = g + ((uint32_t)__builtin_ctz(bad) >> 3);
                                          if (at < first_bad) first_bad = at;
                                      }
                                  });
                    }
                    g0 += R;
                    qc += __shfl(qi, 63, 64), tc += __shfl(ti, 63, 64);
                    prev_last = __shfl(letter, 63, 64);
                }
                // the lanes' parts into lane 0 (all lanes, in fact)
                unsigned long long tq = T.trimmed.q, tt = T.trimmed.t, tcl = T.trimmed.cols, cs = cost, nb = n_bad, fb = first_bad;
                if (__ballot(n_bad != 0ull) != 0ull) {  // (rare: a pair with a bad column)
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        nb += __shfl_xor(nb, o, 64);
                        const unsigned long long f2 = __shfl_xor(fb, o, 64);
                        fb = f2 < fb ? f2 : fb;
                    }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    fl |= __shfl_xor(fl, o, 64);
                    cs = chk_sat_add(cs, __shfl_xor(cs, o, 64));
                    tq += __shfl_xor(tq, o, 64), tt += __shfl_xor(tt, o, 64), tcl += __shfl_xor(tcl, o, 64);
                    T.stats.align_len += __shfl_xor(T.stats.align_len, o, 64);
                    T.stats.matches += __shfl_xor(T.stats.matches, o, 64);
                    T.stats.gaps += __shfl_xor(T.stats.gaps, o, 64);
                    T.stats.gap_regions += __shfl_xor(T.stats.gap_regions, o, 64);
                }
                if (lane == 0) {
                    T.flags = fl, T.cost = cs, T.n_bad = nb, T.first_bad = fb;
                    T.all     = AltSums{g0, qc, tc};
                    T.trimmed = AltSums{tcl, tq, tt};
                    const ChkRec rec = {r[REC_SCORE], r[REC_ALIGN_LEN], r[REC_MATCHES], r[REC_GAPS], r[REC_GAP_REGIONS],
                                        (int32_t)r[REC_QBEGIN], (int32_t)r[REC_QEND], (int32_t)r[REC_TBEGIN], (int32_t)r[REC_TEND]};
                    chk_finish<PACKED>(K.rule, rec, T, q_len, t_len, window, out);
                }
            }
        }
        if (lane == 0) {
            uint32_t *dst = K.chk + i * CHK_WORDS;
            if (K.vec != 0u) {
                reinterpret_cast<uint4 *>(dst)[0] = make_uint4(out[0], out[1], out[2], out[3]);
                reinterpret_cast<uint4 *>(dst)[1] = make_uint4(out[4], out[5], out[6], out[7]);
            } else {
                for (uint32_t k = 0; k < CHK_WORDS; k++) dst[k] = out[k];
            }
            if (K.pass != nullptr) K.pass[i] = chk_pass((int32_t)status, out[CHK_W_FLAGS], K.mask);
            if (status == ST_OK && (out[CHK_W_FLAGS] & K.mask) != 0u) flagged++;
        }
    }
    if (lane == 0 && flagged != 0u) atomicAdd(&K.ctl[CHK_FLAGGED], (unsigned long long)flagged);
}

__global__ __launch_bounds__(256) void wfa_check_kernel(const ChkParams K) {
    chk_wave_pass<false>(K, [&](uint64_t i, uint32_t, uint32_t) {
        const uint8_t *blob = static_cast<const uint8_t *>(K.seq);
        return AltByteSeq{blob + K.q_off[i], blob + K.t_off[i]};
    });
}

__global__ __launch_bounds__(256) void wfa_check_pk_kernel(const ChkParams K) {
    chk_wave_pass<true>(K, [&](uint64_t i, uint32_t q_len, uint32_t t_len) {
        const uint32_t *words = static_cast<const uint32_t *>(K.seq);
        return AltPkSeq{words + K.q_off[i], words + K.t_off[i], q_len, t_len, 0u, 0u, K.q_rc != nullptr && K.q_rc[i] != 0};
    });
}

namespace {

// what every pass of a call shares, its scratch in ctx->cig included
int cig_params(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap, uint64_t n, int only_aligned, void *d_off,
               CigParams *out) {
    const uint32_t n_blocks = (uint32_t)((n + CIG_PER_BLOCK - 1) / CIG_PER_BLOCK);
    // layout of ctx->cig (bytes): counters | blk_sum[n_blocks] | range[n]
    const uint64_t o_blk = CIG_CTL_WORDS * 8, o_rng = o_blk + 8ull * n_blocks;
    int rc = ensure(ctx, ctx->cig, o_rng + 8ull * n);
    if (rc) return rc;
    char *const sb = static_cast<char *>(ctx->cig.p);
    CigParams   C{};
    C.rec = static_cast<const uint32_t *>(d_rec), C.ops = static_cast<const uint64_t *>(d_ops), C.ops_cap = ops_cap, C.n = n;
    C.only_aligned = only_aligned ? 1u : 0u;
    C.text_off = static_cast<uint64_t *>(d_off);
    C.ctl = reinterpret_cast<unsigned long long *>(sb), C.blk_sum = reinterpret_cast<uint64_t *>(sb + o_blk);
    C.range = reinterpret_cast<uint2 *>(sb + o_rng);
    *out = C;
    return WFAHIP_OK;
}

// WFAHIP_DEBUG_TIMING=1 (diagnostics, as in the host entry): the passes' hipEvent times on stderr
struct Stamps {
    hipEvent_t ev[5] = {};
    bool       on    = std::getenv("WFAHIP_DEBUG_TIMING") != nullptr;
    ~Stamps() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void mark(int k, hipStream_t s) {
        if (on && (ev[k] || hipEventCreate(&ev[k]) == hipSuccess)) (void)hipEventRecord(ev[k], s);
    }
    float ms(int a, int b) {
        float v = 0;
        return ev[a] && ev[b] && hipEventElapsedTime(&v, ev[a], ev[b]) == hipSuccess ? v : -1.f;
    }
};

// the three passes on stream st: len(grid) launches the length kernel of a wave per pair, write(grid) the one that writes.
// Returns WFAHIP_OK with *total set and the bytes written; WFAHIP_ERR_OOM (total > cap) with *total set, the offsets filled and no
// byte written; WFAHIP_ERR_BAD_ARG when the length kernel raised CIG_BAD_RANGE, no byte written either.
template <class Len, class Write>
int cig_passes(wfahip_ctx *ctx, const CigParams &C, uint64_t cap, uint64_t *total, hipStream_t st, const char *what, Len &&len,
               Write &&write) {
    const uint64_t n         = C.n;
    const uint32_t n_blocks  = (uint32_t)((n + CIG_PER_BLOCK - 1) / CIG_PER_BLOCK);
    const uint32_t pair_grid = (uint32_t)((n + 3) / 4);
    Stamps stamps;
    HIP_TRY(hipMemsetAsync(C.ctl, 0, CIG_CTL_WORDS * 8, st));
    stamps.mark(0, st);
    len(pair_grid);
    stamps.mark(1, st);
    hipLaunchKernelGGL(wfa_cigar_scan_blocks, dim3(n_blocks), dim3(CIG_SCAN_BLOCK), 0, st, C);
    hipLaunchKernelGGL(wfa_cigar_scan_sums, dim3(1), dim3(1024), 0, st, C, n_blocks);
    if (n > CIG_PER_BLOCK) hipLaunchKernelGGL(wfa_cigar_scan_add, dim3((uint32_t)((n - CIG_PER_BLOCK + 255) / 256)), dim3(256), 0, st, C);
    HIP_TRY(hipGetLastError());
    stamps.mark(2, st);
    // (through the context's pinned block: a pageable copy of 64 bytes costs 0.3 ms)
    HIP_TRY(hipMemcpyAsync(ctx->hpin + HPIN_CTRL, C.ctl, CIG_CTL_WORDS * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    uint64_t hc[CIG_CTL_WORDS];
    std::memcpy(hc, ctx->hpin + HPIN_CTRL, sizeof hc);
    if (hc[CIG_BAD_RANGE] != 0) return WFAHIP_ERR_BAD_ARG;
    *total = hc[CIG_TOTAL];
    if (hc[CIG_TOTAL] > cap) return WFAHIP_ERR_OOM;
    if (hc[CIG_TOTAL] == 0) return WFAHIP_OK;
    stamps.mark(3, st);
    write(pair_grid);
    HIP_TRY(hipGetLastError());
    stamps.mark(4, st);
    HIP_TRY(hipStreamSynchronize(st));
    if (stamps.on)
        std::fprintf(stderr, "[wfahip] %s: %llu pairs, %llu bytes: len %.4f ms, scan %.4f ms, write %.4f ms\n", what, (unsigned long long)n,
                     (unsigned long long)hc[CIG_TOTAL], stamps.ms(0, 1), stamps.ms(1, 2), stamps.ms(3, 4));
    return WFAHIP_OK;
}

int cigar_device_impl(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap, uint64_t n, int only_aligned, void *d_text,
                      uint64_t text_cap, void *d_text_off, uint64_t *total, hipStream_t st) {
    CigParams C{};
    const int rc = cig_params(ctx, d_rec, d_ops, ops_cap, n, only_aligned, d_text_off, &C);
    if (rc) return rc;
    C.text = static_cast<uint8_t *>(d_text);
    return cig_passes(
        ctx, C, text_cap, total, st, "cigar text",
        [&](uint32_t grid) { hipLaunchKernelGGL(wfa_cigar_len_kernel, dim3(grid), dim3(256), 0, st, C); },
        [&](uint32_t grid) { hipLaunchKernelGGL(wfa_cigar_write_kernel, dim3(grid), dim3(256), 0, st, C); });
}

// the rows' three passes; the bytes of a call are those of ONE plane (the three hold the same number)
int altext_device_impl(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap, const void *d_seq_blob, uint64_t blob_bytes,
                       const void *d_q_off, const void *d_q_len, const void *d_t_off, const void *d_t_len, uint64_t n, int only_aligned,
                       void *d_q_row, void *d_a_row, void *d_t_row, uint64_t row_cap, void *d_row_off, uint64_t *total, hipStream_t st) {
    AltParams A{};
    const int rc = cig_params(ctx, d_rec, d_ops, ops_cap, n, only_aligned, d_row_off, &A.C);
    if (rc) return rc;
    A.blob = static_cast<const uint8_t *>(d_seq_blob), A.blob_bytes = blob_bytes;
    A.q_off = static_cast<const uint64_t *>(d_q_off), A.t_off = static_cast<const uint64_t *>(d_t_off);
    A.q_len = static_cast<const uint32_t *>(d_q_len), A.t_len = static_cast<const uint32_t *>(d_t_len);
    A.q_row = static_cast<uint8_t *>(d_q_row), A.a_row = static_cast<uint8_t *>(d_a_row), A.t_row = static_cast<uint8_t *>(d_t_row);
    A.dwords = ((reinterpret_cast<uintptr_t>(d_q_row) | reinterpret_cast<uintptr_t>(d_a_row) | reinterpret_cast<uintptr_t>(d_t_row)) & 3u) == 0u;
    return cig_passes(
        ctx, A.C, row_cap, total, st, "alignment text",
        [&](uint32_t grid) { hipLaunchKernelGGL(wfa_altext_len_kernel, dim3(grid), dim3(256), 0, st, A); },
        [&](uint32_t grid) { hipLaunchKernelGGL(wfa_altext_write_kernel, dim3(grid), dim3(256), 0, st, A); });
}

// the rows from packed words: the same three passes over AltPkParams
int altext_pk_device_impl(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap, const void *d_packed, uint64_t n_words,
                          const void *d_q_woff, const void *d_q_len, const void *d_t_woff, const void *d_t_len, const void *d_q_rc, uint64_t n,
                          int only_aligned, void *d_q_row, void *d_a_row, void *d_t_row, uint64_t row_cap, void *d_row_off, uint64_t *total,
                          hipStream_t st) {
    AltPkParams A{};
    const int   rc = cig_params(ctx, d_rec, d_ops, ops_cap, n, only_aligned, d_row_off, &A.C);
    if (rc) return rc;
    A.words = static_cast<const uint32_t *>(d_packed), A.n_words = n_words;
    A.q_woff = static_cast<const uint64_t *>(d_q_woff), A.t_woff = static_cast<const uint64_t *>(d_t_woff);
    A.q_len = static_cast<const uint32_t *>(d_q_len), A.t_len = static_cast<const uint32_t *>(d_t_len);
    A.q_rc  = static_cast<const uint8_t *>(d_q_rc);
    A.q_row = static_cast<uint8_t *>(d_q_row), A.a_row = static_cast<uint8_t *>(d_a_row), A.t_row = static_cast<uint8_t *>(d_t_row);
    A.dwords = ((reinterpret_cast<uintptr_t>(d_q_row) | reinterpret_cast<uintptr_t>(d_a_row) | reinterpret_cast<uintptr_t>(d_t_row)) & 3u) == 0u;
    return cig_passes(
        ctx, A.C, row_cap, total, st, "alignment text packed",
        [&](uint32_t grid) { hipLaunchKernelGGL(wfa_altext_pk_len_kernel, dim3(grid), dim3(256), 0, st, A); },
        [&](uint32_t grid) { hipLaunchKernelGGL(wfa_altext_pk_write_kernel, dim3(grid), dim3(256), 0, st, A); });
}

// the difference string's three passes: the rows' parameters with the text in C.text (the planes stay null)
int diff_device_impl(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap, const void *d_seq_blob, uint64_t blob_bytes,
                     const void *d_q_off, const void *d_q_len, const void *d_t_off, const void *d_t_len, uint64_t n, int only_aligned,
                     void *d_text, uint64_t text_cap, void *d_text_off, uint64_t *total, hipStream_t st) {
    AltParams A{};
    const int rc = cig_params(ctx, d_rec, d_ops, ops_cap, n, only_aligned, d_text_off, &A.C);
    if (rc) return rc;
    A.C.text = static_cast<uint8_t *>(d_text);
    A.blob = static_cast<const uint8_t *>(d_seq_blob), A.blob_bytes = blob_bytes;
    A.q_off = static_cast<const uint64_t *>(d_q_off), A.t_off = static_cast<const uint64_t *>(d_t_off);
    A.q_len = static_cast<const uint32_t *>(d_q_len), A.t_len = static_cast<const uint32_t *>(d_t_len);
    A.dwords = (reinterpret_cast<uintptr_t>(d_text) & 3u) == 0u;
    return cig_passes(
        ctx, A.C, text_cap, total, st, "diff text",
        [&](uint32_t grid) { hipLaunchKernelGGL(wfa_diff_len_kernel, dim3(grid), dim3(256), 0, st, A); },
        [&](uint32_t grid) { hipLaunchKernelGGL(wfa_diff_write_kernel, dim3(grid), dim3(256), 0, st, A); });
}

int diff_pk_device_impl(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap, const void *d_packed, uint64_t n_words,
                        const void *d_q_woff, const void *d_q_len, const void *d_t_woff, const void *d_t_len, const void *d_q_rc, uint64_t n,
                        int only_aligned, void *d_text, uint64_t text_cap, void *d_text_off, uint64_t *total, hipStream_t st) {
    AltPkParams A{};
    const int   rc = cig_params(ctx, d_rec, d_ops, ops_cap, n, only_aligned, d_text_off, &A.C);
    if (rc) return rc;
    A.C.text = static_cast<uint8_t *>(d_text);
    A.words = static_cast<const uint32_t *>(d_packed), A.n_words = n_words;
    A.q_woff = static_cast<const uint64_t *>(d_q_woff), A.t_woff = static_cast<const uint64_t *>(d_t_woff);
    A.q_len = static_cast<const uint32_t *>(d_q_len), A.t_len = static_cast<const uint32_t *>(d_t_len);
    A.q_rc   = static_cast<const uint8_t *>(d_q_rc);
    A.dwords = (reinterpret_cast<uintptr_t>(d_text) & 3u) == 0u;
    return cig_passes(
        ctx, A.C, text_cap, total, st, "diff text packed",
        [&](uint32_t grid) { hipLaunchKernelGGL(wfa_diff_pk_len_kernel, dim3(grid), dim3(256), 0, st, A); },
        [&](uint32_t grid) { hipLaunchKernelGGL(wfa_diff_pk_write_kernel, dim3(grid), dim3(256), 0, st, A); });
}

// what the two row entries share: seq_args_ok is the verdict on the pointers of the sequences (nothing before impl dereferences the
// context), impl(st, &total) runs the three passes
template <class Impl>
int altext_entry(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap, bool seq_args_ok, uint64_t n_pairs, void *d_q_row,
                 void *d_a_row, void *d_t_row, uint64_t row_cap, void *d_row_off, uint64_t *row_needed, hipStream_t st, Impl &&impl) {
    if (!ctx || (n_pairs && (!d_rec || !d_row_off)) || !seq_args_ok) return WFAHIP_ERR_BAD_ARG;
    if ((!d_ops && ops_cap) || ((!d_q_row || !d_a_row || !d_t_row) && row_cap)) return WFAHIP_ERR_BAD_ARG;
    if (n_pairs > 0xFFFFFFF0ull) return WFAHIP_ERR_BAD_ARG;  // (align_device's limit: no entry leaves records of more pairs)
    if (row_needed) *row_needed = 0;
    if (n_pairs == 0 && !d_row_off) return WFAHIP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (!st) st = ctx->stream;
    if (n_pairs == 0) {
        HIP_TRY(hipMemsetAsync(d_row_off, 0, 8, st));
        HIP_TRY(hipStreamSynchronize(st));
        return WFAHIP_OK;
    }
    uint64_t  total = 0;
    const int rc    = impl(st, &total);
    if (row_needed && (rc == WFAHIP_OK || rc == WFAHIP_ERR_OOM)) *row_needed = total;
    return rc;
}

int altext_device_entry(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap, const void *d_seq_blob, uint64_t blob_bytes,
                        const void *d_q_off, const void *d_q_len, const void *d_t_off, const void *d_t_len, uint64_t n_pairs, int only_aligned,
                        void *d_q_row, void *d_a_row, void *d_t_row, uint64_t row_cap, void *d_row_off, uint64_t *row_needed,
                        hipStream_t st) {
    const bool seq_ok = !(n_pairs && (!d_q_off || !d_q_len || !d_t_off || !d_t_len)) && !(!d_seq_blob && blob_bytes);
    return altext_entry(ctx, d_rec, d_ops, ops_cap, seq_ok, n_pairs, d_q_row, d_a_row, d_t_row, row_cap, d_row_off, row_needed, st,
                        [&](hipStream_t s, uint64_t *total) {
                            return altext_device_impl(ctx, d_rec, d_ops, ops_cap, d_seq_blob, blob_bytes, d_q_off, d_q_len, d_t_off, d_t_len,
                                                      n_pairs, only_aligned, d_q_row, d_a_row, d_t_row, row_cap, d_row_off, total, s);
                        });
}

int altext_pk_device_entry(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap, const void *d_packed, uint64_t n_words,
                           const void *d_q_woff, const void *d_q_len, const void *d_t_woff, const void *d_t_len, const void *d_q_rc,
                           uint64_t n_pairs, int only_aligned, void *d_q_row, void *d_a_row, void *d_t_row, uint64_t row_cap, void *d_row_off,
                           uint64_t *row_needed, hipStream_t st) {
    const bool seq_ok = !(n_pairs && (!d_q_woff || !d_q_len || !d_t_woff || !d_t_len)) && !(!d_packed && n_words);
    return altext_entry(ctx, d_rec, d_ops, ops_cap, seq_ok, n_pairs, d_q_row, d_a_row, d_t_row, row_cap, d_row_off, row_needed, st,
                        [&](hipStream_t s, uint64_t *total) {
                            return altext_pk_device_impl(ctx, d_rec, d_ops, ops_cap, d_packed, n_words, d_q_woff, d_q_len, d_t_woff, d_t_len,
                                                         d_q_rc, n_pairs, only_aligned, d_q_row, d_a_row, d_t_row, row_cap, d_row_off, total, s);
                        });
}

// what the entries that write ONE text share (the CIGAR text, the difference string): seq_args_ok is the verdict on the pointers of
// the sequences (true where there are none), impl(st, &total) runs the three passes
template <class Impl>
int text_entry(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap, bool seq_args_ok, uint64_t n_pairs, void *d_text,
               uint64_t text_cap, void *d_text_off, uint64_t *text_needed, hipStream_t st, Impl &&impl) {
    // (nothing in these checks dereferences the context)
    if (!ctx || (n_pairs && (!d_rec || !d_text_off)) || !seq_args_ok || (!d_ops && ops_cap) || (!d_text && text_cap)) return WFAHIP_ERR_BAD_ARG;
    if (n_pairs > 0xFFFFFFF0ull) return WFAHIP_ERR_BAD_ARG;  // (align_device's limit: no entry leaves records of more pairs)
    if (text_needed) *text_needed = 0;
    if (n_pairs == 0 && !d_text_off) return WFAHIP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (!st) st = ctx->stream;
    if (n_pairs == 0) {
        HIP_TRY(hipMemsetAsync(d_text_off, 0, 8, st));
        HIP_TRY(hipStreamSynchronize(st));
        return WFAHIP_OK;
    }
    uint64_t  total = 0;
    const int rc    = impl(st, &total);
    if (text_needed && (rc == WFAHIP_OK || rc == WFAHIP_ERR_OOM)) *text_needed = total;
    return rc;
}

int cigar_text_device_entry(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap, uint64_t n_pairs, int only_aligned,
                            void *d_text, uint64_t text_cap, void *d_text_off, uint64_t *text_needed, hipStream_t st) {
    return text_entry(ctx, d_rec, d_ops, ops_cap, true, n_pairs, d_text, text_cap, d_text_off, text_needed, st,
                      [&](hipStream_t s, uint64_t *total) {
                          return cigar_device_impl(ctx, d_rec, d_ops, ops_cap, n_pairs, only_aligned, d_text, text_cap, d_text_off, total, s);
                      });
}

int diff_device_entry(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap, const void *d_seq_blob, uint64_t blob_bytes,
                      const void *d_q_off, const void *d_q_len, const void *d_t_off, const void *d_t_len, uint64_t n_pairs, int only_aligned,
                      void *d_text, uint64_t text_cap, void *d_text_off, uint64_t *text_needed, hipStream_t st) {
    const bool seq_ok = !(n_pairs && (!d_q_off || !d_q_len || !d_t_off || !d_t_len)) && !(!d_seq_blob && blob_bytes);
    return text_entry(ctx, d_rec, d_ops, ops_cap, seq_ok, n_pairs, d_text, text_cap, d_text_off, text_needed, st,
                      [&](hipStream_t s, uint64_t *total) {
                          return diff_device_impl(ctx, d_rec, d_ops, ops_cap, d_seq_blob, blob_bytes, d_q_off, d_q_len, d_t_off, d_t_len, n_pairs,
                                                  only_aligned, d_text, text_cap, d_text_off, total, s);
                      });
}

int diff_pk_device_entry(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap, const void *d_packed, uint64_t n_words,
                         const void *d_q_woff, const void *d_q_len, const void *d_t_woff, const void *d_t_len, const void *d_q_rc,
                         uint64_t n_pairs, int only_aligned, void *d_text, uint64_t text_cap, void *d_text_off, uint64_t *text_needed,
                         hipStream_t st) {
    const bool seq_ok = !(n_pairs && (!d_q_woff || !d_q_len || !d_t_woff || !d_t_len)) && !(!d_packed && n_words);
    return text_entry(ctx, d_rec, d_ops, ops_cap, seq_ok, n_pairs, d_text, text_cap, d_text_off, text_needed, st,
                      [&](hipStream_t s, uint64_t *total) {
                          return diff_pk_device_impl(ctx, d_rec, d_ops, ops_cap, d_packed, n_words, d_q_woff, d_q_len, d_t_woff, d_t_len, d_q_rc,
                                                     n_pairs, only_aligned, d_text, text_cap, d_text_off, total, s);
                      });
}

// the pileup's two passes on stream st: len(grid) launches the length kernel with the waves striding over the pairs, pile(grid) the
// kernel of a wave per pair that adds.  WFAHIP_ERR_BAD_ARG when the length kernel raised CIG_BAD_RANGE: no counter is touched.
template <class Len, class Pile>
int pile_passes(wfahip_ctx *ctx, const CigParams &C, uint64_t *n_piled, hipStream_t st, const char *what, Len &&len, Pile &&pile) {
    Stamps stamps;
    HIP_TRY(hipMemsetAsync(C.ctl, 0, CIG_CTL_WORDS * 8, st));
    stamps.mark(0, st);
    len((uint32_t)std::min<uint64_t>((C.n + 3) / 4, CHK_MAX_GRID));
    HIP_TRY(hipGetLastError());
    stamps.mark(1, st);
    // (through the context's pinned block, as the text entries fetch their counters)
    HIP_TRY(hipMemcpyAsync(ctx->hpin + HPIN_CTRL, C.ctl, CIG_CTL_WORDS * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    uint64_t hc[CIG_CTL_WORDS];
    std::memcpy(hc, ctx->hpin + HPIN_CTRL, sizeof hc);
    if (hc[CIG_BAD_RANGE] != 0) return WFAHIP_ERR_BAD_ARG;
    if (n_piled) *n_piled = hc[CIG_TOTAL];
    if (hc[CIG_TOTAL] == 0) return WFAHIP_OK;
    stamps.mark(3, st);
    pile((uint32_t)((C.n + 3) / 4));
    HIP_TRY(hipGetLastError());
    stamps.mark(4, st);
    HIP_TRY(hipStreamSynchronize(st));
    if (stamps.on)
        std::fprintf(stderr, "[wfahip] %s: %llu pairs, %llu piled: len %.4f ms, pile %.4f ms\n", what, (unsigned long long)C.n,
                     (unsigned long long)hc[CIG_TOTAL], stamps.ms(0, 1), stamps.ms(3, 4));
    return WFAHIP_OK;
}

// the two device entries of the pileup: d_seq is the blob or the words, seq_size blob_bytes or n_words, the offsets byte or word
// offsets, d_q_rc only the words'
int pile_device_entry(wfahip_ctx *ctx, bool packed, const void *d_rec, const void *d_ops, uint64_t ops_cap, const void *d_seq,
                      uint64_t seq_size, const void *d_q_off, const void *d_q_len, const void *d_t_off, const void *d_t_len, const void *d_q_rc,
                      uint64_t n, int only_aligned, uint64_t pile_at, uint64_t pile_n, void *d_counts, uint64_t *n_piled, hipStream_t st) {
    // (nothing in these checks dereferences the context)
    if (!ctx || (n && (!d_rec || !d_q_off || !d_q_len || !d_t_off || !d_t_len)) || (!d_ops && ops_cap) || (!d_seq && seq_size) ||
        (!d_counts && pile_n))
        return WFAHIP_ERR_BAD_ARG;
    if (pile_n > PILE_MAX_N || n > 0xFFFFFFF0ull) return WFAHIP_ERR_BAD_ARG;  // (align_device's limit: no entry leaves records of more pairs)
    if (n_piled) *n_piled = 0;
    if (n == 0 || pile_n == 0) return WFAHIP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (!st) st = ctx->stream;
    const PileWin   W      = {pile_at, pile_n};
    uint32_t *const counts = static_cast<uint32_t *>(d_counts);
    if (packed) {
        AltPkParams A{};
        const int   rc = cig_params(ctx, d_rec, d_ops, ops_cap, n, only_aligned, nullptr, &A.C);
        if (rc) return rc;
        A.words = static_cast<const uint32_t *>(d_seq), A.n_words = seq_size;
        A.q_woff = static_cast<const uint64_t *>(d_q_off), A.t_woff = static_cast<const uint64_t *>(d_t_off);
        A.q_len = static_cast<const uint32_t *>(d_q_len), A.t_len = static_cast<const uint32_t *>(d_t_len);
        A.q_rc = static_cast<const uint8_t *>(d_q_rc);
        return pile_passes(
            ctx, A.C, n_piled, st, "pileup packed",
            [&](uint32_t grid) { hipLaunchKernelGGL(wfa_pile_pk_len_kernel, dim3(grid), dim3(256), 0, st, A); },
            [&](uint32_t grid) { hipLaunchKernelGGL(wfa_pile_pk_kernel, dim3(grid), dim3(256), 0, st, A, W, counts); });
    }
    AltParams A{};
    const int rc = cig_params(ctx, d_rec, d_ops, ops_cap, n, only_aligned, nullptr, &A.C);
    if (rc) return rc;
    A.blob = static_cast<const uint8_t *>(d_seq), A.blob_bytes = seq_size;
    A.q_off = static_cast<const uint64_t *>(d_q_off), A.t_off = static_cast<const uint64_t *>(d_t_off);
    A.q_len = static_cast<const uint32_t *>(d_q_len), A.t_len = static_cast<const uint32_t *>(d_t_len);
    return pile_passes(
        ctx, A.C, n_piled, st, "pileup",
        [&](uint32_t grid) { hipLaunchKernelGGL(wfa_pile_len_kernel, dim3(grid), dim3(256), 0, st, A); },
        [&](uint32_t grid) { hipLaunchKernelGGL(wfa_pile_kernel, dim3(grid), dim3(256), 0, st, A, W, counts); });
}

void cigars_zero(wfahip_cigars *c) { std::memset(c, 0, sizeof *c); }

// the ops of pair i of host results that render: *count of them at *ops (none for a pair that is not OK).  false: an OK pair whose
// ops leave [0, n_ops); none of them is read.
bool host_pair_ops(const wfahip_results *r, uint64_t i, bool trim, const uint64_t **ops, uint32_t *count) {
    *ops = nullptr, *count = 0u;
    if (r->status[i] != WFAHIP_PAIR_OK) return true;
    const uint32_t len = r->ops_len[i];
    if (len > r->n_ops || r->ops_off[i] > r->n_ops - len) return false;  // (compared without a sum that could wrap)
    if (len == 0u) return true;
    uint32_t first;
    cig_range(r->ops + r->ops_off[i], len, trim, &first, count);
    *ops = r->ops + r->ops_off[i] + first;
    return true;
}

// the host renderers' plan: n_threads threads over contiguous ranges of pairs, twice.  len(i, &bytes) gives the bytes of pair i
// (false: the pair is invalid, the call WFAHIP_ERR_BAD_ARG); the ranges' sums give their bases; alloc(total) makes the output
// (not called for a total of 0; false: WFAHIP_ERR_OOM); write(i, at) renders a pair with bytes at its offset.  *off_out is
// malloc'd, n + 1 offsets; nothing is left allocated on an error.
template <class Len, class Alloc, class Write>
int host_render(uint64_t n, int n_threads, uint64_t **off_out, uint64_t *total_out, Len &&len, Alloc &&alloc, Write &&write) {
    if (n > (SIZE_MAX / 8) - 1) return WFAHIP_ERR_OOM;
    uint64_t *const off = static_cast<uint64_t *>(std::malloc((size_t)(n + 1) * 8));
    if (!off) return WFAHIP_ERR_OOM;
    off[n] = 0;
    const unsigned        T   = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(1, n_threads), n));
    const uint64_t        per = T ? (n + T - 1) / T : 0;
    std::vector<uint64_t> part(T + 1, 0);
    std::atomic<int>      bad{0};
    uint64_t *const       part_p = part.data();
    parallel_ranges(0, T, T, [&, part_p](uint64_t t0, uint64_t t1) {
        for (uint64_t t = t0; t < t1; t++) {
            const uint64_t a = std::min(n, t * per), b = std::min(n, a + per);
            uint64_t       sum = 0;
            for (uint64_t i = a; i < b; i++) {
                off[i] = 0;
                if (!len(i, &off[i])) bad = 1, off[i] = 0;
                sum += off[i];
            }
            part_p[t + 1] = sum;
        }
    });
    if (bad) {
        std::free(off);
        return WFAHIP_ERR_BAD_ARG;
    }
    for (unsigned t = 0; t < T; t++) part[t + 1] += part[t];
    const uint64_t total = part[T];
    if (total && !alloc(total)) {
        std::free(off);
        return WFAHIP_ERR_OOM;
    }
    parallel_ranges(0, T, T, [&, part_p](uint64_t t0, uint64_t t1) {
        for (uint64_t t = t0; t < t1; t++) {
            const uint64_t a = std::min(n, t * per), b = std::min(n, a + per);
            uint64_t       run = part_p[t];
            for (uint64_t i = a; i < b; i++) {
                const uint64_t bytes = off[i];
                off[i]               = run;
                if (bytes) write(i, run);
                run += bytes;
            }
        }
    });
    off[n]     = total;
    *off_out   = off;
    *total_out = total;
    return WFAHIP_OK;
}

int cigar_text_host(const wfahip_results *r, int only_aligned, int n_threads, wfahip_cigars *out) {
    if (out) cigars_zero(out);
    if (!r || !out) return WFAHIP_ERR_BAD_ARG;
    const uint64_t n = r->n;
    if (n && (!r->status || !r->ops_off || !r->ops_len)) return WFAHIP_ERR_BAD_ARG;
    if (!r->ops && r->n_ops) return WFAHIP_ERR_BAD_ARG;
    char      *text = nullptr;
    uint64_t  *off = nullptr, total = 0;
    const bool trim = only_aligned != 0;
    const int  rc   = host_render(
        n, n_threads, &off, &total,
        [&](uint64_t i, uint64_t *bytes) {
            uint32_t        count;
            const uint64_t *ops;
            if (!host_pair_ops(r, i, trim, &ops, &count)) return false;
            *bytes = count ? cig_text_bytes(ops, count) : 0;
            return true;
        },
        [&](uint64_t bytes) { return (text = static_cast<char *>(std::malloc((size_t)bytes))) != nullptr; },
        [&](uint64_t i, uint64_t at) {
            uint32_t        count;
            const uint64_t *ops;
            (void)host_pair_ops(r, i, trim, &ops, &count);
            cig_text_write(ops, count, reinterpret_cast<uint8_t *>(text) + at);
        });
    if (rc) return rc;
    out->n       = n;
    out->n_bytes = total;
    out->text    = text;
    out->off     = off;
    return WFAHIP_OK;
}

void align_texts_zero(wfahip_align_texts *t) { std::memset(t, 0, sizeof *t); }

// the host row renderers' plan.  seq_args_ok is the verdict on the pointers of the sequences (with r->n > 0 the four arrays, and the
// blob or the words); window(i, trim, &w) gives the windows of pair i -- asked only for an OK pair with an op that renders --, false
// where they fail; rows_write(i, ops, count, w, q_row, a_row, t_row) renders the pair.  columns_only: the windows of a pair whose
// ops have no column are not asked for (the packed entry; the byte entry checks every pair with an op in its range).
// a pair's rendering ops, its windows and the size of what it renders; false where wfa_altext.hpp's checks fail.  sums(ops, count,
// &size) gives the ops' AltSums and that size -- the columns of the rows, the bytes of the difference string.  ONE copy of the checks
// for the host renderers of both.
template <class Window, class Sums>
bool host_pair_checked(const wfahip_results *r, uint64_t i, bool trim, bool columns_only, Window &&window, Sums &&sums, const uint64_t **ops,
                       uint32_t *count, AltWindow *w, uint64_t *size) {
    if (!host_pair_ops(r, i, trim, ops, count)) return false;
    *size = 0;
    if (*count == 0u) return true;
    uint64_t      sz = 0;
    const AltSums s  = sums(*ops, *count, &sz);
    if (columns_only && s.cols == 0) return true;
    if (!window(i, trim, w) || !alt_fits(s, *w)) return false;
    *size = s.cols != 0 ? sz : 0;
    return true;
}

template <class Window, class RowsWrite>
int alignment_text_host_impl(const wfahip_results *r, bool seq_args_ok, bool columns_only, int only_aligned, int n_threads,
                             wfahip_align_texts *out, Window &&window, RowsWrite &&rows_write) {
    if (out) align_texts_zero(out);
    if (!r || !out) return WFAHIP_ERR_BAD_ARG;
    const uint64_t n = r->n;
    if (n && (!r->status || !r->ops_off || !r->ops_len)) return WFAHIP_ERR_BAD_ARG;
    if (n && only_aligned && (!r->qbegin || !r->qend || !r->tbegin || !r->tend)) return WFAHIP_ERR_BAD_ARG;
    if ((!r->ops && r->n_ops) || !seq_args_ok) return WFAHIP_ERR_BAD_ARG;
    char      *rows[3] = {nullptr, nullptr, nullptr};
    uint64_t  *off = nullptr, total = 0;
    const bool trim = only_aligned != 0;
    // a pair's rendering ops and windows; false where wfa_altext.hpp's checks fail
    const auto pair = [&](uint64_t i, const uint64_t **ops, uint32_t *count, AltWindow *w, uint64_t *cols) {
        return host_pair_checked(
            r, i, trim, columns_only, window,
            [](const uint64_t *o, uint32_t c, uint64_t *size) {
                const AltSums s = alt_sums(o, c);
                *size           = s.cols;
                return s;
            },
            ops, count, w, cols);
    };
    const int rc = host_render(
        n, n_threads, &off, &total,
        [&](uint64_t i, uint64_t *bytes) {
            uint32_t        count;
            const uint64_t *ops;
            AltWindow       w;
            return pair(i, &ops, &count, &w, bytes);
        },
        [&](uint64_t bytes) {
            for (char *&p : rows) p = static_cast<char *>(std::malloc((size_t)bytes));
            if (rows[0] && rows[1] && rows[2]) return true;
            for (char *&p : rows) std::free(p), p = nullptr;
            return false;
        },
        [&](uint64_t i, uint64_t at) {
            uint32_t        count;
            const uint64_t *ops;
            AltWindow       w;
            uint64_t        cols;
            (void)pair(i, &ops, &count, &w, &cols);
            rows_write(i, ops, count, w, reinterpret_cast<uint8_t *>(rows[0]) + at, reinterpret_cast<uint8_t *>(rows[1]) + at,
                       reinterpret_cast<uint8_t *>(rows[2]) + at);
        });
    if (rc) return rc;
    out->n       = n;
    out->n_bytes = total;
    out->q_row = rows[0], out->a_row = rows[1], out->t_row = rows[2];
    out->off = off;
    return WFAHIP_OK;
}

int alignment_text_host(const wfahip_results *r, const uint8_t *seq_blob, uint64_t blob_bytes, const uint64_t *q_off, const uint32_t *q_len,
                        const uint64_t *t_off, const uint32_t *t_len, int only_aligned, int n_threads, wfahip_align_texts *out) {
    const bool seq_ok = r && !(r->n && (!q_off || !q_len || !t_off || !t_len)) && !(!seq_blob && blob_bytes);
    return alignment_text_host_impl(
        r, seq_ok, false, only_aligned, n_threads, out,
        [&](uint64_t i, bool trim, AltWindow *w) {
            return alt_window(trim, blob_bytes, q_off[i], q_len[i], t_off[i], t_len[i], trim ? r->qbegin[i] : 0, trim ? r->qend[i] : 0,
                              trim ? r->tbegin[i] : 0, trim ? r->tend[i] : 0, w);
        },
        [&](uint64_t, const uint64_t *ops, uint32_t count, const AltWindow &w, uint8_t *q_row, uint8_t *a_row, uint8_t *t_row) {
            alt_rows_write(ops, count, seq_blob + w.q_at, seq_blob + w.t_at, q_row, a_row, t_row);
        });
}

int alignment_text_packed_host(const wfahip_results *r, const uint32_t *packed, uint64_t n_words, const uint64_t *q_woff,
                               const uint32_t *q_len, const uint64_t *t_woff, const uint32_t *t_len, const uint8_t *q_rc, int only_aligned,
                               int n_threads, wfahip_align_texts *out) {
    const bool seq_ok = r && !(r->n && (!q_woff || !q_len || !t_woff || !t_len)) && !(!packed && n_words);
    return alignment_text_host_impl(
        r, seq_ok, true, only_aligned, n_threads, out,
        [&](uint64_t i, bool trim, AltWindow *w) {
            return alt_pk_window(trim, n_words, q_woff[i], q_len[i], t_woff[i], t_len[i], trim ? r->qbegin[i] : 0, trim ? r->qend[i] : 0,
                                 trim ? r->tbegin[i] : 0, trim ? r->tend[i] : 0, w);
        },
        [&](uint64_t i, const uint64_t *ops, uint32_t count, const AltWindow &w, uint8_t *q_row, uint8_t *a_row, uint8_t *t_row) {
            alt_pk_rows_write(ops, count, packed + q_woff[i], q_len[i], q_rc != nullptr && q_rc[i] != 0, (uint32_t)w.q_at, packed + t_woff[i],
                              t_len[i], (uint32_t)w.t_at, q_row, a_row, t_row);
        });
}

// the host renderers of the difference string: alignment_text_host_impl's plan with one text in place of three rows.  make_seq(i, w)
// gives wfa_diff.hpp's reader of pair i's windows.
template <class Window, class MakeSeq>
int diff_text_host_impl(const wfahip_results *r, bool seq_args_ok, bool columns_only, int only_aligned, int n_threads, wfahip_cigars *out,
                        Window &&window, MakeSeq &&make_seq) {
    if (out) cigars_zero(out);
    if (!r || !out) return WFAHIP_ERR_BAD_ARG;
    const uint64_t n = r->n;
    if (n && (!r->status || !r->ops_off || !r->ops_len)) return WFAHIP_ERR_BAD_ARG;
    if (n && only_aligned && (!r->qbegin || !r->qend || !r->tbegin || !r->tend)) return WFAHIP_ERR_BAD_ARG;
    if ((!r->ops && r->n_ops) || !seq_args_ok) return WFAHIP_ERR_BAD_ARG;
    char      *text = nullptr;
    uint64_t  *off = nullptr, total = 0;
    const bool trim = only_aligned != 0;
    const auto pair = [&](uint64_t i, const uint64_t **ops, uint32_t *count, AltWindow *w, uint64_t *bytes) {
        return host_pair_checked(
            r, i, trim, columns_only, window,
            [](const uint64_t *o, uint32_t c, uint64_t *size) {
                const DiffSums s = diff_sums(o, c);
                *size            = s.bytes;
                return s.a;
            },
            ops, count, w, bytes);
    };
    const int rc = host_render(
        n, n_threads, &off, &total,
        [&](uint64_t i, uint64_t *bytes) {
            uint32_t        count;
            const uint64_t *ops;
            AltWindow       w;
            return pair(i, &ops, &count, &w, bytes);
        },
        [&](uint64_t bytes) { return (text = static_cast<char *>(std::malloc((size_t)bytes))) != nullptr; },
        [&](uint64_t i, uint64_t at) {
            uint32_t        count;
            const uint64_t *ops;
            AltWindow       w;
            uint64_t        bytes;
            (void)pair(i, &ops, &count, &w, &bytes);
            diff_write(ops, count, make_seq(i, w), reinterpret_cast<uint8_t *>(text) + at);
        });
    if (rc) return rc;
    out->n       = n;
    out->n_bytes = total;
    out->text    = text;
    out->off     = off;
    return WFAHIP_OK;
}

int diff_text_host(const wfahip_results *r, const uint8_t *seq_blob, uint64_t blob_bytes, const uint64_t *q_off, const uint32_t *q_len,
                   const uint64_t *t_off, const uint32_t *t_len, int only_aligned, int n_threads, wfahip_cigars *out) {
    const bool seq_ok = r && !(r->n && (!q_off || !q_len || !t_off || !t_len)) && !(!seq_blob && blob_bytes);
    return diff_text_host_impl(
        r, seq_ok, false, only_aligned, n_threads, out,
        [&](uint64_t i, bool trim, AltWindow *w) {
            return alt_window(trim, blob_bytes, q_off[i], q_len[i], t_off[i], t_len[i], trim ? r->qbegin[i] : 0, trim ? r->qend[i] : 0,
                              trim ? r->tbegin[i] : 0, trim ? r->tend[i] : 0, w);
        },
        [&](uint64_t, const AltWindow &w) { return DiffByteSeq{seq_blob + w.q_at, seq_blob + w.t_at}; });
}

int diff_text_packed_host(const wfahip_results *r, const uint32_t *packed, uint64_t n_words, const uint64_t *q_woff, const uint32_t *q_len,
                          const uint64_t *t_woff, const uint32_t *t_len, const uint8_t *q_rc, int only_aligned, int n_threads,
                          wfahip_cigars *out) {
    const bool seq_ok = r && !(r->n && (!q_woff || !q_len || !t_woff || !t_len)) && !(!packed && n_words);
    return diff_text_host_impl(
        r, seq_ok, true, only_aligned, n_threads, out,
        [&](uint64_t i, bool trim, AltWindow *w) {
            return alt_pk_window(trim, n_words, q_woff[i], q_len[i], t_woff[i], t_len[i], trim ? r->qbegin[i] : 0, trim ? r->qend[i] : 0,
                                 trim ? r->tbegin[i] : 0, trim ? r->tend[i] : 0, w);
        },
        [&](uint64_t i, const AltWindow &w) {
            return DiffPkSeq{packed + q_woff[i], packed + t_woff[i], q_len[i], t_len[i], (uint32_t)w.q_at, (uint32_t)w.t_at,
                             q_rc != nullptr && q_rc[i] != 0};
        });
}

// the host entries of the pileup: every pair through the renderers' checks first (host_pair_checked: a failed one leaves counts
// untouched), then the adds -- n_threads threads over contiguous ranges of pairs, relaxed atomic adds because pairs share targets.
// seq_args_ok and window as alignment_text_host_impl takes them; make_seq(i, w, &T0) gives wfa_pile.hpp's reader of pair i's query
// window and the coordinate of its target window's first base.
template <class Window, class MakeSeq>
int pileup_host_impl(const wfahip_results *r, bool seq_args_ok, bool columns_only, int only_aligned, int n_threads, uint64_t pile_at,
                     uint64_t pile_n, uint32_t *counts, uint64_t *n_piled, Window &&window, MakeSeq &&make_seq) {
    if (!r) return WFAHIP_ERR_BAD_ARG;
    const uint64_t n = r->n;
    if (n && (!r->status || !r->ops_off || !r->ops_len)) return WFAHIP_ERR_BAD_ARG;
    if (n && only_aligned && (!r->qbegin || !r->qend || !r->tbegin || !r->tend)) return WFAHIP_ERR_BAD_ARG;
    if ((!r->ops && r->n_ops) || !seq_args_ok || (!counts && pile_n) || pile_n > PILE_MAX_N) return WFAHIP_ERR_BAD_ARG;
    if (n_piled) *n_piled = 0;
    if (n == 0 || pile_n == 0) return WFAHIP_OK;
    const bool trim = only_aligned != 0;
    const auto pair = [&](uint64_t i, const uint64_t **ops, uint32_t *count, AltWindow *w, uint64_t *cols) {
        return host_pair_checked(
            r, i, trim, columns_only, window,
            [](const uint64_t *o, uint32_t c, uint64_t *size) {
                const AltSums s = alt_sums(o, c);
                *size           = s.cols;
                return s;
            },
            ops, count, w, cols);
    };
    const unsigned        T = (unsigned)std::max(1, n_threads);
    std::atomic<int>      bad{0};
    std::atomic<uint64_t> piled{0};
    parallel_ranges(0, n, T, [&](uint64_t a, uint64_t b) {
        uint64_t mine = 0;
        for (uint64_t i = a; i < b; i++) {
            uint32_t        count;
            const uint64_t *ops;
            AltWindow       w;
            uint64_t        cols = 0;
            if (!pair(i, &ops, &count, &w, &cols)) bad = 1;
            else if (cols != 0) mine++;
        }
        piled += mine;
    });
    if (bad) return WFAHIP_ERR_BAD_ARG;
    const PileWin W = {pile_at, pile_n};
    parallel_ranges(0, n, T, [&](uint64_t a, uint64_t b) {
        for (uint64_t i = a; i < b; i++) {
            uint32_t        count;
            const uint64_t *ops;
            AltWindow       w;
            uint64_t        cols = 0;
            (void)pair(i, &ops, &count, &w, &cols);
            if (cols == 0) continue;
            uint64_t   T0;
            const auto S = make_seq(i, w, &T0);
            pile_pair(ops, count, S, T0, w.t_n, W,
                      [&](uint64_t idx, uint32_t word, uint32_t v) { (void)__atomic_fetch_add(counts + idx * PILE_WORDS + word, v, __ATOMIC_RELAXED); });
        }
    });
    if (n_piled) *n_piled = piled;
    return WFAHIP_OK;
}

int pileup_host(const wfahip_results *r, const uint8_t *seq_blob, uint64_t blob_bytes, const uint64_t *q_off, const uint32_t *q_len,
                const uint64_t *t_off, const uint32_t *t_len, int only_aligned, int n_threads, uint64_t pile_at, uint64_t pile_n,
                uint32_t *counts, uint64_t *n_piled) {
    const bool seq_ok = r && !(r->n && (!q_off || !q_len || !t_off || !t_len)) && !(!seq_blob && blob_bytes);
    return pileup_host_impl(
        r, seq_ok, false, only_aligned, n_threads, pile_at, pile_n, counts, n_piled,
        [&](uint64_t i, bool trim, AltWindow *w) {
            return alt_window(trim, blob_bytes, q_off[i], q_len[i], t_off[i], t_len[i], trim ? r->qbegin[i] : 0, trim ? r->qend[i] : 0,
                              trim ? r->tbegin[i] : 0, trim ? r->tend[i] : 0, w);
        },
        [&](uint64_t, const AltWindow &w, uint64_t *T0) {
            *T0 = w.t_at;
            return PileByteSeq{seq_blob + w.q_at};
        });
}

int pileup_packed_host(const wfahip_results *r, const uint32_t *packed, uint64_t n_words, const uint64_t *q_woff, const uint32_t *q_len,
                       const uint64_t *t_woff, const uint32_t *t_len, const uint8_t *q_rc, int only_aligned, int n_threads, uint64_t pile_at,
                       uint64_t pile_n, uint32_t *counts, uint64_t *n_piled) {
    const bool seq_ok = r && !(r->n && (!q_woff || !q_len || !t_woff || !t_len)) && !(!packed && n_words);
    return pileup_host_impl(
        r, seq_ok, true, only_aligned, n_threads, pile_at, pile_n, counts, n_piled,
        [&](uint64_t i, bool trim, AltWindow *w) {
            return alt_pk_window(trim, n_words, q_woff[i], q_len[i], t_woff[i], t_len[i], trim ? r->qbegin[i] : 0, trim ? r->qend[i] : 0,
                                 trim ? r->tbegin[i] : 0, trim ? r->tend[i] : 0, w);
        },
        [&](uint64_t i, const AltWindow &w, uint64_t *T0) {
            *T0 = 16ull * t_woff[i] + w.t_at;
            return PilePkSeq{packed + q_woff[i], q_len[i], (uint32_t)w.q_at, q_rc != nullptr && q_rc[i] != 0};
        });
}

// ---- the check (wfa_check.hpp): the device entries and the host entries

// what the four entries refuse before anything is dereferenced but the params (seq: the blob or the words)
int check_args(const void *ctx_or_results, const wfahip_params *p, const void *chk, uint64_t n, bool per_pair_ok, const void *ops,
               uint64_t ops_cap, const void *seq, uint64_t seq_size) {
    if (!ctx_or_results || !p || !chk) return WFAHIP_ERR_BAD_ARG;
    if (n && !per_pair_ok) return WFAHIP_ERR_BAD_ARG;
    if ((!ops && ops_cap) || (!seq && seq_size)) return WFAHIP_ERR_BAD_ARG;
    if (n > 0xFFFFFFF0ull) return WFAHIP_ERR_BAD_ARG;  // (align_device's limit: no entry leaves records of more pairs)
    return check_params(p);
}

int check_device_entry(wfahip_ctx *ctx, const wfahip_params *p, bool packed, const void *d_rec, const void *d_ops, uint64_t ops_cap,
                       const void *d_seq, uint64_t seq_size, const void *d_q_off, const void *d_q_len, const void *d_t_off,
                       const void *d_t_len, const void *d_q_rc, uint64_t n, uint32_t flag_mask, void *d_chk, void *d_pass,
                       uint64_t *n_flagged, hipStream_t st) {
    int rc = check_args(ctx, p, d_chk, n, d_rec && d_q_off && d_q_len && d_t_off && d_t_len, d_ops, ops_cap, d_seq, seq_size);
    if (rc) return rc;
    if (n_flagged) *n_flagged = 0;
    if (n == 0) return WFAHIP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (!st) st = ctx->stream;
    if ((rc = ensure(ctx, ctx->cig, CIG_CTL_WORDS * 8))) return rc;
    ChkParams K{};
    K.rec = static_cast<const uint32_t *>(d_rec), K.ops = static_cast<const uint64_t *>(d_ops), K.ops_cap = ops_cap, K.n = n;
    K.rule = ChkRule{p->mismatch, p->gap_open, p->gap_ext, p->global_alignment != 0};
    K.mask = flag_mask;
    K.seq = d_seq, K.seq_size = seq_size;
    K.q_off = static_cast<const uint64_t *>(d_q_off), K.t_off = static_cast<const uint64_t *>(d_t_off);
    K.q_len = static_cast<const uint32_t *>(d_q_len), K.t_len = static_cast<const uint32_t *>(d_t_len);
    K.q_rc = static_cast<const uint8_t *>(d_q_rc);
    K.chk = static_cast<uint32_t *>(d_chk), K.pass = static_cast<int32_t *>(d_pass);
    K.vec = (reinterpret_cast<uintptr_t>(d_chk) & 15u) == 0u;
    K.ctl = static_cast<unsigned long long *>(ctx->cig.p);
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 3) / 4, CHK_MAX_GRID);
    Stamps         stamps;
    HIP_TRY(hipMemsetAsync(K.ctl, 0, CIG_CTL_WORDS * 8, st));
    stamps.mark(0, st);
    if (packed) hipLaunchKernelGGL(wfa_check_pk_kernel, dim3(grid), dim3(256), 0, st, K);
    else hipLaunchKernelGGL(wfa_check_kernel, dim3(grid), dim3(256), 0, st, K);
    HIP_TRY(hipGetLastError());
    stamps.mark(1, st);
    // (through the context's pinned block, as the text entries fetch their counters)
    HIP_TRY(hipMemcpyAsync(ctx->hpin + HPIN_CTRL, K.ctl, CIG_CTL_WORDS * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    uint64_t hc[CIG_CTL_WORDS];
    std::memcpy(hc, ctx->hpin + HPIN_CTRL, sizeof hc);
    if (n_flagged) *n_flagged = hc[CHK_FLAGGED];
    if (stamps.on)
        std::fprintf(stderr, "[wfahip] %s: %llu pairs, %llu flagged: kernel %.4f ms\n", packed ? "check alignments packed" : "check alignments",
                     (unsigned long long)n, (unsigned long long)hc[CHK_FLAGGED], stamps.ms(0, 1));
    return WFAHIP_OK;
}

int check_host_entry(const wfahip_results *r, const wfahip_params *p, bool packed, const void *seq, uint64_t seq_size, const uint64_t *q_off,
                     const uint32_t *q_len, const uint64_t *t_off, const uint32_t *t_len, const uint8_t *q_rc, uint32_t flag_mask,
                     int n_threads, uint32_t *chk, int32_t *pass, uint64_t *n_flagged) {
    const uint64_t n  = r ? r->n : 0;
    const bool     ok = r && r->status && r->score && r->tbegin && r->tend && r->qbegin && r->qend && r->align_len && r->matches && r->gaps &&
                    r->gap_regions && r->ops_off && r->ops_len && q_off && q_len && t_off && t_len;
    const int rc = check_args(r, p, chk, n, ok, r ? r->ops : nullptr, r ? r->n_ops : 0, seq, seq_size);
    if (rc) return rc;
    if (n_flagged) *n_flagged = 0;
    if (n == 0) return WFAHIP_OK;
    const ChkRule         R = {p->mismatch, p->gap_open, p->gap_ext, p->global_alignment != 0};
    std::atomic<uint64_t> flagged{0};
    parallel_ranges(0, n, (unsigned)std::max(1, n_threads), [&](uint64_t a, uint64_t b) {
        uint64_t mine = 0;
        for (uint64_t i = a; i < b; i++) {
            uint32_t *out = chk + i * CHK_WORDS;
            if (r->status[i] != WFAHIP_PAIR_OK) {
                chk_unread(false, out);
            } else if (chk_ops_range(r->ops_off[i], r->ops_len[i], r->n_ops)) {
                chk_unread(true, out);
            } else {
                const ChkRec    rec = {r->score[i], r->align_len[i], r->matches[i], r->gaps[i], r->gap_regions[i],
                                       r->qbegin[i], r->qend[i], r->tbegin[i], r->tend[i]};
                const uint64_t *ops = r->ops_len[i] ? r->ops + r->ops_off[i] : nullptr;
                if (packed) {
                    const uint32_t *words = static_cast<const uint32_t *>(seq);
                    chk_pair<true>(
                        R, rec, ops, r->ops_len[i], q_len[i], t_len[i],
                        [&](bool trim, AltWindow *w) {
                            return alt_pk_window(trim, seq_size, q_off[i], q_len[i], t_off[i], t_len[i], rec.qbegin, rec.qend, rec.tbegin, rec.tend, w);
                        },
                        [&]() { return ChkPkSeq{words + q_off[i], words + t_off[i], q_len[i], t_len[i], q_rc != nullptr && q_rc[i] != 0}; }, out);
                } else {
                    const uint8_t *blob = static_cast<const uint8_t *>(seq);
                    chk_pair<false>(
                        R, rec, ops, r->ops_len[i], q_len[i], t_len[i],
                        [&](bool trim, AltWindow *w) {
                            return alt_window(trim, seq_size, q_off[i], q_len[i], t_off[i], t_len[i], rec.qbegin, rec.qend, rec.tbegin, rec.tend, w);
                        },
                        [&]() { return ChkByteSeq{blob + q_off[i], blob + t_off[i]}; }, out);
                }
            }
            if (pass) pass[i] = chk_pass(r->status[i], out[CHK_W_FLAGS], flag_mask);
            if (r->status[i] == WFAHIP_PAIR_OK && (out[CHK_W_FLAGS] & flag_mask) != 0u) mine++;
        }
        flagged += mine;
    });
    if (n_flagged) *n_flagged = flagged;
    return WFAHIP_OK;
}

// wfahip_align_batch_text: the plain path of wfahip_align_batch with the text kernels in place of the result assembly
int align_batch_text_impl(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *seq_blob, uint64_t blob_bytes, const uint64_t *q_off,
                          const uint32_t *q_len, const uint64_t *t_off, const uint32_t *t_len, uint64_t n_pairs, int only_aligned,
                          wfahip_results *out, wfahip_cigars *cig) {
    if (cig) cigars_zero(cig);
    if (!ctx || !out || !cig) return WFAHIP_ERR_BAD_ARG;
    results_zero(out);
    int rc = check_params(p);
    if (rc) return rc;
    if (n_pairs == 0) {
        cig->off = static_cast<uint64_t *>(std::calloc(1, 8));
        return cig->off ? WFAHIP_OK : WFAHIP_ERR_OOM;
    }
    if (!q_off || !q_len || !t_off || !t_len || (!seq_blob && blob_bytes)) return WFAHIP_ERR_BAD_ARG;
    if (n_pairs > 0xFFFFFFF0ull) return WFAHIP_ERR_BAD_ARG;
    // (the last of the whole-call errors: nothing above or in this loop dereferences the context)
    uint32_t max_len = 1;
    uint64_t sum_len = 0;
    for (uint64_t i = 0; i < n_pairs; i++) {
        if (q_len[i] <= WFAHIP_MAX_SEQ_LEN && t_len[i] <= WFAHIP_MAX_SEQ_LEN && q_len[i] && t_len[i]) {
            if (q_off[i] > blob_bytes || q_len[i] > blob_bytes - q_off[i] || t_off[i] > blob_bytes || t_len[i] > blob_bytes - t_off[i])
                return WFAHIP_ERR_BAD_ARG;
            max_len = std::max(max_len, std::max(q_len[i], t_len[i]));
            sum_len += (uint64_t)q_len[i] + t_len[i];
        }
    }
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // ---- one upload (+32 bytes: aligned dword loads at the blob's tail stay inside the allocation)
    if ((rc = ensure(ctx, ctx->in_blob, blob_bytes + 32))) return rc;
    if ((rc = ensure(ctx, ctx->in_qoff, n_pairs * 8))) return rc;
    if ((rc = ensure(ctx, ctx->in_toff, n_pairs * 8))) return rc;
    if ((rc = ensure(ctx, ctx->in_qlen, n_pairs * 4))) return rc;
    if ((rc = ensure(ctx, ctx->in_tlen, n_pairs * 4))) return rc;
    if ((rc = ensure(ctx, ctx->out_rec, n_pairs * REC_WORDS * 4))) return rc;
    if (blob_bytes) HIP_TRY(hipMemcpyAsync(ctx->in_blob.p, seq_blob, blob_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->in_qoff.p, q_off, n_pairs * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->in_toff.p, t_off, n_pairs * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->in_qlen.p, q_len, n_pairs * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->in_tlen.p, t_len, n_pairs * 4, hipMemcpyHostToDevice, st));
    // ---- the alignment.  CIGAR ops are merged runs: a first guess of (n+m)/4 + 8 per pair, grown on demand (the host entry's rule)
    uint64_t ops_cap = sum_len / 4 + 8 * n_pairs + 1024;
    for (int attempt = 0; attempt < 6; attempt++) {
        if ((rc = ensure(ctx, ctx->out_ops, ops_cap * 8))) return rc;
        uint64_t needed = 0;
        rc = align_device(ctx, p, ctx->in_blob.p, blob_bytes, ctx->in_qoff.p, ctx->in_qlen.p, ctx->in_toff.p, ctx->in_tlen.p, n_pairs, max_len,
                          ctx->out_rec.p, ctx->out_ops.p, ops_cap, &needed, st, false);
        if (rc == WFAHIP_ERR_OOM && needed > ops_cap) {
            ops_cap = needed + needed / 3 + 1024;
            continue;
        }
        break;
    }
    if (rc) return rc;
    // ---- the text: sized by the first two passes, written by a second call once its buffer is there (the lengths are cheap to
    // make again; an op renders to at most 11 bytes, but a buffer for that bound would be three times the text of typical ops)
    if ((rc = ensure(ctx, ctx->cig_off, (n_pairs + 1) * 8))) return rc;
    uint64_t total = 0;
    rc = cigar_device_impl(ctx, ctx->out_rec.p, ctx->out_ops.p, ops_cap, n_pairs, only_aligned, ctx->cig_text.p, ctx->cig_text.bytes,
                           ctx->cig_off.p, &total, st);
    if (rc == WFAHIP_ERR_OOM && total > ctx->cig_text.bytes) {
        if ((rc = ensure(ctx, ctx->cig_text, total + total / 8))) return rc;
        rc = cigar_device_impl(ctx, ctx->out_rec.p, ctx->out_ops.p, ops_cap, n_pairs, only_aligned, ctx->cig_text.p, ctx->cig_text.bytes,
                               ctx->cig_off.p, &total, st);
    }
    if (rc) return rc == WFAHIP_ERR_BAD_ARG ? WFAHIP_ERR_INTERNAL : rc;  // (the records are the library's own)
    // ---- one download: records, offsets, text
    std::vector<uint32_t> rec((size_t)n_pairs * REC_WORDS);
    cig->off = static_cast<uint64_t *>(std::malloc((size_t)(n_pairs + 1) * 8));
    if (total) cig->text = static_cast<char *>(std::malloc((size_t)total));
    const auto fail = [&](int code) {
        wfahip_results_free(out);
        std::free(cig->text), std::free(cig->off);
        cigars_zero(cig);
        return code;
    };
    if (!cig->off || (total && !cig->text)) return fail(WFAHIP_ERR_OOM);
    hipError_t e = hipMemcpyAsync(rec.data(), ctx->out_rec.p, rec.size() * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(cig->off, ctx->cig_off.p, (size_t)(n_pairs + 1) * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && total) e = hipMemcpyAsync(cig->text, ctx->cig_text.p, (size_t)total, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        std::snprintf(ctx->last_error, sizeof ctx->last_error, "%s: download -> %s", __FILE__, hipGetErrorString(e));
        return fail(e == hipErrorOutOfMemory ? WFAHIP_ERR_OOM : WFAHIP_ERR_HIP);
    }
    cig->n = n_pairs, cig->n_bytes = total;
    // ---- the records unpacked (unpack_results' field rules: every field of a pair that is not OK is 0; here ops_off is 0 too)
    out->n = n_pairs;
#define ALLOC(field, type)                                                \
    out->field = static_cast<type *>(std::calloc(n_pairs, sizeof(type))); \
    if (!out->field) return fail(WFAHIP_ERR_OOM);
    ALLOC(status, int32_t) ALLOC(score, uint32_t) ALLOC(tbegin, int32_t) ALLOC(tend, int32_t)
    ALLOC(qbegin, int32_t) ALLOC(qend, int32_t) ALLOC(align_len, uint32_t) ALLOC(matches, uint32_t)
    ALLOC(gaps, uint32_t) ALLOC(gap_regions, uint32_t) ALLOC(ops_off, uint64_t) ALLOC(ops_len, uint32_t)
#undef ALLOC
    uint64_t cells = 0;
    for (uint64_t i = 0; i < n_pairs; i++) {
        const uint32_t *r  = &rec[i * REC_WORDS];
        const uint32_t  s  = r[REC_STATUS];
        out->status[i]     = (s == ST_OK || s == ST_EMPTY || s == ST_TOO_LONG || s == ST_OVER_MAX) ? (int32_t)s : WFAHIP_PAIR_NO_MEMORY;
        if (s != ST_OK) continue;
        out->score[i]       = r[REC_SCORE];
        out->tbegin[i]      = (int32_t)r[REC_TBEGIN];
        out->tend[i]        = (int32_t)r[REC_TEND];
        out->qbegin[i]      = (int32_t)r[REC_QBEGIN];
        out->qend[i]        = (int32_t)r[REC_QEND];
        out->align_len[i]   = r[REC_ALIGN_LEN];
        out->matches[i]     = r[REC_MATCHES];
        out->gaps[i]        = r[REC_GAPS];
        out->gap_regions[i] = r[REC_GAP_REGIONS];
        out->ops_len[i]     = r[REC_OPS_LEN];
        cells += (uint64_t)r[REC_CELLS_LO] | ((uint64_t)r[REC_CELLS_HI] << 32);
    }
    ctx->timing.cells_stored = cells;
    return WFAHIP_OK;
}

}  // namespace

extern "C" int wfahip_cigar_text_device(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap, uint64_t n_pairs,
                                        int only_aligned, void *d_text, uint64_t text_cap, void *d_text_off, uint64_t *text_needed,
                                        void *stream) {
    WFAHIP_GUARD(cigar_text_device_entry(ctx, d_rec, d_ops, ops_cap, n_pairs, only_aligned, d_text, text_cap, d_text_off, text_needed,
                                         static_cast<hipStream_t>(stream)))
}

extern "C" int wfahip_cigar_text(const wfahip_results *r, int only_aligned, int n_threads, wfahip_cigars *out) {
    WFAHIP_GUARD(cigar_text_host(r, only_aligned, n_threads, out))
}

extern "C" void wfahip_cigars_free(wfahip_cigars *c) {
    if (!c) return;
    std::free(c->text), std::free(c->off);
    cigars_zero(c);
}

extern "C" int wfahip_alignment_text_device(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap, const void *d_seq_blob,
                                            uint64_t blob_bytes, const void *d_q_off, const void *d_q_len, const void *d_t_off,
                                            const void *d_t_len, uint64_t n_pairs, int only_aligned, void *d_q_row, void *d_a_row,
                                            void *d_t_row, uint64_t row_cap, void *d_row_off, uint64_t *row_needed, void *stream) {
    WFAHIP_GUARD(altext_device_entry(ctx, d_rec, d_ops, ops_cap, d_seq_blob, blob_bytes, d_q_off, d_q_len, d_t_off, d_t_len, n_pairs,
                                     only_aligned, d_q_row, d_a_row, d_t_row, row_cap, d_row_off, row_needed, static_cast<hipStream_t>(stream)))
}

extern "C" int wfahip_alignment_text(const wfahip_results *r, const uint8_t *seq_blob, uint64_t blob_bytes, const uint64_t *q_off,
                                     const uint32_t *q_len, const uint64_t *t_off, const uint32_t *t_len, int only_aligned, int n_threads,
                                     wfahip_align_texts *out) {
    WFAHIP_GUARD(alignment_text_host(r, seq_blob, blob_bytes, q_off, q_len, t_off, t_len, only_aligned, n_threads, out))
}

extern "C" int wfahip_alignment_text_packed_device(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap,
                                                   const void *d_packed, uint64_t n_words, const void *d_q_woff, const void *d_q_len,
                                                   const void *d_t_woff, const void *d_t_len, const void *d_q_rc, uint64_t n_pairs,
                                                   int only_aligned, void *d_q_row, void *d_a_row, void *d_t_row, uint64_t row_cap,
                                                   void *d_row_off, uint64_t *row_needed, void *stream) {
    WFAHIP_GUARD(altext_pk_device_entry(ctx, d_rec, d_ops, ops_cap, d_packed, n_words, d_q_woff, d_q_len, d_t_woff, d_t_len, d_q_rc, n_pairs,
                                        only_aligned, d_q_row, d_a_row, d_t_row, row_cap, d_row_off, row_needed,
                                        static_cast<hipStream_t>(stream)))
}

extern "C" int wfahip_alignment_text_packed(const wfahip_results *r, const uint32_t *packed, uint64_t n_words, const uint64_t *q_woff,
                                            const uint32_t *q_len, const uint64_t *t_woff, const uint32_t *t_len, const uint8_t *q_rc,
                                            int only_aligned, int n_threads, wfahip_align_texts *out) {
    WFAHIP_GUARD(alignment_text_packed_host(r, packed, n_words, q_woff, q_len, t_woff, t_len, q_rc, only_aligned, n_threads, out))
}

extern "C" int wfahip_diff_text_device(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap, const void *d_seq_blob,
                                       uint64_t blob_bytes, const void *d_q_off, const void *d_q_len, const void *d_t_off, const void *d_t_len,
                                       uint64_t n_pairs, int only_aligned, void *d_text, uint64_t text_cap, void *d_text_off,
                                       uint64_t *text_needed, void *stream) {
    WFAHIP_GUARD(diff_device_entry(ctx, d_rec, d_ops, ops_cap, d_seq_blob, blob_bytes, d_q_off, d_q_len, d_t_off, d_t_len, n_pairs, only_aligned,
                                   d_text, text_cap, d_text_off, text_needed, static_cast<hipStream_t>(stream)))
}

extern "C" int wfahip_diff_text_packed_device(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap, const void *d_packed,
                                              uint64_t n_words, const void *d_q_woff, const void *d_q_len, const void *d_t_woff,
                                              const void *d_t_len, const void *d_q_rc, uint64_t n_pairs, int only_aligned, void *d_text,
                                              uint64_t text_cap, void *d_text_off, uint64_t *text_needed, void *stream) {
    WFAHIP_GUARD(diff_pk_device_entry(ctx, d_rec, d_ops, ops_cap, d_packed, n_words, d_q_woff, d_q_len, d_t_woff, d_t_len, d_q_rc, n_pairs,
                                      only_aligned, d_text, text_cap, d_text_off, text_needed, static_cast<hipStream_t>(stream)))
}

extern "C" int wfahip_diff_text(const wfahip_results *r, const uint8_t *seq_blob, uint64_t blob_bytes, const uint64_t *q_off,
                                const uint32_t *q_len, const uint64_t *t_off, const uint32_t *t_len, int only_aligned, int n_threads,
                                wfahip_cigars *out) {
    WFAHIP_GUARD(diff_text_host(r, seq_blob, blob_bytes, q_off, q_len, t_off, t_len, only_aligned, n_threads, out))
}

extern "C" int wfahip_diff_text_packed(const wfahip_results *r, const uint32_t *packed, uint64_t n_words, const uint64_t *q_woff,
                                       const uint32_t *q_len, const uint64_t *t_woff, const uint32_t *t_len, const uint8_t *q_rc,
                                       int only_aligned, int n_threads, wfahip_cigars *out) {
    WFAHIP_GUARD(diff_text_packed_host(r, packed, n_words, q_woff, q_len, t_woff, t_len, q_rc, only_aligned, n_threads, out))
}

extern "C" int wfahip_pileup_device(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap, const void *d_seq_blob,
                                    uint64_t blob_bytes, const void *d_q_off, const void *d_q_len, const void *d_t_off, const void *d_t_len,
                                    uint64_t n_pairs, int only_aligned, uint64_t pile_at, uint64_t pile_n, void *d_counts, uint64_t *n_piled,
                                    void *stream) {
    WFAHIP_GUARD(pile_device_entry(ctx, false, d_rec, d_ops, ops_cap, d_seq_blob, blob_bytes, d_q_off, d_q_len, d_t_off, d_t_len, nullptr,
                                   n_pairs, only_aligned, pile_at, pile_n, d_counts, n_piled, static_cast<hipStream_t>(stream)))
}

extern "C" int wfahip_pileup_packed_device(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap, const void *d_packed,
                                           uint64_t n_words, const void *d_q_woff, const void *d_q_len, const void *d_t_woff,
                                           const void *d_t_len, const void *d_q_rc, uint64_t n_pairs, int only_aligned, uint64_t pile_at,
                                           uint64_t pile_n, void *d_counts, uint64_t *n_piled, void *stream) {
    WFAHIP_GUARD(pile_device_entry(ctx, true, d_rec, d_ops, ops_cap, d_packed, n_words, d_q_woff, d_q_len, d_t_woff, d_t_len, d_q_rc, n_pairs,
                                   only_aligned, pile_at, pile_n, d_counts, n_piled, static_cast<hipStream_t>(stream)))
}

extern "C" int wfahip_pileup(const wfahip_results *r, const uint8_t *seq_blob, uint64_t blob_bytes, const uint64_t *q_off,
                             const uint32_t *q_len, const uint64_t *t_off, const uint32_t *t_len, int only_aligned, int n_threads,
                             uint64_t pile_at, uint64_t pile_n, uint32_t *counts, uint64_t *n_piled) {
    WFAHIP_GUARD(pileup_host(r, seq_blob, blob_bytes, q_off, q_len, t_off, t_len, only_aligned, n_threads, pile_at, pile_n, counts, n_piled))
}

extern "C" int wfahip_pileup_packed(const wfahip_results *r, const uint32_t *packed, uint64_t n_words, const uint64_t *q_woff,
                                    const uint32_t *q_len, const uint64_t *t_woff, const uint32_t *t_len, const uint8_t *q_rc,
                                    int only_aligned, int n_threads, uint64_t pile_at, uint64_t pile_n, uint32_t *counts, uint64_t *n_piled) {
    WFAHIP_GUARD(pileup_packed_host(r, packed, n_words, q_woff, q_len, t_woff, t_len, q_rc, only_aligned, n_threads, pile_at, pile_n, counts,
                                    n_piled))
}

extern "C" void wfahip_align_texts_free(wfahip_align_texts *t) {
    if (!t) return;
    std::free(t->q_row), std::free(t->a_row), std::free(t->t_row), std::free(t->off);
    align_texts_zero(t);
}

extern "C" int wfahip_align_batch_text(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *seq_blob, uint64_t blob_bytes,
                                       const uint64_t *q_off, const uint32_t *q_len, const uint64_t *t_off, const uint32_t *t_len,
                                       uint64_t n_pairs, int only_aligned, wfahip_results *out, wfahip_cigars *cig) {
    WFAHIP_GUARD(align_batch_text_impl(ctx, p, seq_blob, blob_bytes, q_off, q_len, t_off, t_len, n_pairs, only_aligned, out, cig))
}

extern "C" int wfahip_check_alignments_device(wfahip_ctx *ctx, const wfahip_params *p, const void *d_rec, const void *d_ops, uint64_t ops_cap,
                                              const void *d_seq_blob, uint64_t blob_bytes, const void *d_q_off, const void *d_q_len,
                                              const void *d_t_off, const void *d_t_len, uint64_t n_pairs, uint32_t flag_mask, void *d_chk,
                                              void *d_pass, uint64_t *n_flagged, void *stream) {
    WFAHIP_GUARD(check_device_entry(ctx, p, false, d_rec, d_ops, ops_cap, d_seq_blob, blob_bytes, d_q_off, d_q_len, d_t_off, d_t_len, nullptr,
                                    n_pairs, flag_mask, d_chk, d_pass, n_flagged, static_cast<hipStream_t>(stream)))
}

extern "C" int wfahip_check_alignments_packed_device(wfahip_ctx *ctx, const wfahip_params *p, const void *d_rec, const void *d_ops,
                                                     uint64_t ops_cap, const void *d_packed, uint64_t n_words, const void *d_q_woff,
                                                     const void *d_q_len, const void *d_t_woff, const void *d_t_len, const void *d_q_rc,
                                                     uint64_t n_pairs, uint32_t flag_mask, void *d_chk, void *d_pass, uint64_t *n_flagged,
                                                     void *stream) {
    WFAHIP_GUARD(check_device_entry(ctx, p, true, d_rec, d_ops, ops_cap, d_packed, n_words, d_q_woff, d_q_len, d_t_woff, d_t_len, d_q_rc,
                                    n_pairs, flag_mask, d_chk, d_pass, n_flagged, static_cast<hipStream_t>(stream)))
}

extern "C" int wfahip_check_alignments(const wfahip_results *r, const wfahip_params *p, const uint8_t *seq_blob, uint64_t blob_bytes,
                                       const uint64_t *q_off, const uint32_t *q_len, const uint64_t *t_off, const uint32_t *t_len,
                                       uint32_t flag_mask, int n_threads, uint32_t *chk, int32_t *pass, uint64_t *n_flagged) {
    WFAHIP_GUARD(check_host_entry(r, p, false, seq_blob, blob_bytes, q_off, q_len, t_off, t_len, nullptr, flag_mask, n_threads, chk, pass,
                                  n_flagged))
}

extern "C" int wfahip_check_alignments_packed(const wfahip_results *r, const wfahip_params *p, const uint32_t *packed, uint64_t n_words,
                                              const uint64_t *q_woff, const uint32_t *q_len, const uint64_t *t_woff, const uint32_t *t_len,
                                              const uint8_t *q_rc, uint32_t flag_mask, int n_threads, uint32_t *chk, int32_t *pass,
                                              uint64_t *n_flagged) {
    WFAHIP_GUARD(check_host_entry(r, p, true, packed, n_words, q_woff, q_len, t_woff, t_len, q_rc, flag_mask, n_threads, chk, pass, n_flagged))
}
