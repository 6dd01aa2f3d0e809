// wfa_check.hpp -- the verdict on one alignment: ONE source of the rule for the kernels (wfa_cigar.hip: wfahip_check_alignments_device,
// wfahip_check_alignments_packed_device) and the host entries (wfahip_check_alignments, wfahip_check_alignments_packed).
//
// A pair's record, its ops and its two sequences give WFAHIP_CHK_WORDS = 8 u32 words: FLAGS, COST, Q_USED, T_USED, N_BAD, FIRST_BAD,
// 0, 0.  The flags state what IS, not what is wrong (the reference's own results raise some of them).  In this order:
//   1. a status other than WFAHIP_PAIR_OK: eight zeros, and nothing else of the pair is read;
//   2. OPS_RANGE: OPS_LEN > ops_cap or OPS_OFF > ops_cap - OPS_LEN: FLAGS = OPS_RANGE | NO_ROWS | NO_ROWS_TRIMMED, the other words
//      0, no op read;
//   3. over all ops: LETTER (a letter outside M X I D H), ZERO (a count of 0), UNMERGED (two neighbours of one letter), NO_M (no 'M'
//      op; an empty op list has none);
//   4. Q_USED / T_USED, the bases the ops consume as alt_kind says, and COST -- x * count for 'X', o + e * count for 'I' 'D' 'H', 0
//      for the rest --, each word min(true value, 0xFFFFFFFF): the bases are 64-bit sums, the cost a saturating 64-bit sum (one op's
//      cost is at most 2^64 - 2^32, and whatever saturates lies above every u32 it is compared with);
//   5. SEQ_RANGE: a sequence leaves the blob or the words (alt_window / alt_pk_window untrimmed): no sequence byte is read, N_BAD = 0,
//      FIRST_BAD = 0xFFFFFFFF;
//   6. Q_OVER / Q_UNDER / T_OVER / T_UNDER: the bases consumed against the sequence's length;
//   7. the 'M' and 'X' columns whose query index is < q_len and whose target index is < t_len: an 'M' column of two different
//      bytes raises M_DIFFERS, an 'X' column of two equal bytes X_EQUAL; N_BAD counts them (saturating) and FIRST_BAD is the index
//      of the first among ALL columns of the untrimmed rows, at most 0xFFFFFFFE, 0xFFFFFFFF when there is none.  Indices never
//      decrease, so these columns are a prefix of the 'M' / 'X' columns: chk_valid says how many of an op's are in it;
//   8. NO_ROWS / NO_ROWS_TRIMMED: wfahip_alignment_text(_packed)_device's checks with only_aligned 0 / 1 fail for the pair --
//      cig_range, alt_sums' sums, alt_window / alt_pk_window and alt_fits themselves, not a restatement;
//   9. global alignment only: COST_OVER (true cost > SCORE), COST_UNDER (true cost < SCORE: the reference's merge of two gaps that
//      were opened separately into one op);
//  10. STAT_ALIGN_LEN / STAT_MATCHES / STAT_GAPS / STAT_GAP_REGIONS: the record's field differs from process() recomputed over the
//      ops (wfa_cigar.go:171-211): u32 wrapping sums over the first to the last 'M' op -- without one, op 0 alone, as the Go loop
//      behaves (nothing for an empty list) --, 'H' in the length and not in the gaps.
// Nothing here needs HIP: the header compiles as plain C++ (tests/check_host_test.cpp).
#pragma once
#include <stdint.h>

#include "wfa_altext_pk.hpp"

namespace wfa {

constexpr uint32_t CHK_WORDS = 8;
enum { CHK_W_FLAGS = 0, CHK_W_COST, CHK_W_Q_USED, CHK_W_T_USED, CHK_W_N_BAD, CHK_W_FIRST_BAD };
// (include/wfa_hip.h: WFAHIP_CHK_*)
constexpr uint32_t CHK_OPS_RANGE = 1u << 0, CHK_LETTER = 1u << 1, CHK_ZERO = 1u << 2, CHK_UNMERGED = 1u << 3, CHK_NO_M = 1u << 4,
                   CHK_SEQ_RANGE = 1u << 5, CHK_Q_OVER = 1u << 6, CHK_Q_UNDER = 1u << 7, CHK_T_OVER = 1u << 8, CHK_T_UNDER = 1u << 9,
                   CHK_M_DIFFERS = 1u << 10, CHK_X_EQUAL = 1u << 11, CHK_NO_ROWS = 1u << 12, CHK_NO_ROWS_TRIMMED = 1u << 13,
                   CHK_COST_OVER = 1u << 14, CHK_COST_UNDER = 1u << 15, CHK_STAT_ALIGN_LEN = 1u << 16, CHK_STAT_MATCHES = 1u << 17,
                   CHK_STAT_GAPS = 1u << 18, CHK_STAT_GAP_REGIONS = 1u << 19, CHK_ALL = (1u << 20) - 1u;
constexpr int32_t  CHK_PAIR_FAILED = 16;  // WFAHIP_PAIR_CHECK_FAILED
constexpr uint32_t CHK_NONE = 0xFFFFFFFFu;  // FIRST_BAD without a bad column

// the penalties and the one option the rule looks at
struct ChkRule {
    uint32_t x, o, e;
    bool     global;
};

// the fields of a record the rule looks at (a device record's words, or the arrays of a wfahip_results)
struct ChkRec {
    uint32_t score, align_len, matches, gaps, gap_regions;
    int32_t  qbegin, qend, tbegin, tend;
};

__host__ __device__ inline uint64_t chk_sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }
__host__ __device__ inline uint32_t chk_sat32(uint64_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }

// step 3's flags of one op; has_prev: there is an op before it, of letter prev
__host__ __device__ inline uint32_t chk_op_flags(uint64_t op, bool has_prev, uint32_t prev) {
    const uint32_t l = (uint32_t)(op >> 32);
    uint32_t       f = 0u;
    if (alt_kind(op) == 0u) f |= CHK_LETTER;  // (alt_kind knows exactly M X I D H)
    if ((uint32_t)op == 0u) f |= CHK_ZERO;
    if (has_prev && l == prev) f |= CHK_UNMERGED;
    return f;
}

// step 4's cost of one op: at most (2^32 - 1)^2 + 2^32 - 1 = 2^64 - 2^32
__host__ __device__ inline uint64_t chk_op_cost(uint64_t op, const ChkRule &R) {
    const uint64_t c = (uint32_t)op;
    switch ((uint32_t)(op >> 32)) {
    case 'X': return (uint64_t)R.x * c;
    case 'I':
    case 'D':
    case 'H': return (uint64_t)R.o + (uint64_t)R.e * c;
    default: return 0ull;
    }
}

// step 10's sums over ops (u32, wrapping)
struct ChkStats {
    uint32_t align_len, matches, gaps, gap_regions;
};

__host__ __device__ inline void chk_stat_add(ChkStats *s, uint64_t op) {
    const uint32_t c = (uint32_t)op, l = (uint32_t)(op >> 32);
    const bool     gap = l == (uint32_t)'I' || l == (uint32_t)'D';
    s->align_len += c;
    s->matches += l == (uint32_t)'M' ? c : 0u;  // (values, not a switch over the fields: the kernels keep them in registers)
    s->gaps += gap ? c : 0u;
    s->gap_regions += gap ? 1u : 0u;
}

// the ops process() sums: [*first, *first + *count) of len ops, given cig_range's trimmed range [m_first, m_first + m_count)
__host__ __device__ inline void chk_stat_range(uint32_t len, uint32_t m_first, uint32_t m_count, uint32_t *first, uint32_t *count) {
    if (m_count != 0u) *first = m_first, *count = m_count;
    else *first = 0u, *count = len != 0u ? 1u : 0u;
}

// step 7: an 'M' or 'X' op?  Its columns are the ones compared.
__host__ __device__ inline bool chk_compares(uint64_t op) { return alt_kind(op) == (ALT_Q | ALT_T); }

// step 7: how many of the first columns of an 'M' / 'X' op of cnt columns, whose first column reads query base qs and target base
// ts (true 64-bit sums), lie inside both sequences
__host__ __device__ inline uint32_t chk_valid(uint32_t cnt, uint64_t qs, uint64_t ts, uint32_t q_len, uint32_t t_len) {
    const uint64_t qn = qs < q_len ? q_len - qs : 0ull, tn = ts < t_len ? t_len - ts : 0ull;
    const uint64_t v  = qn < tn ? qn : tn;
    return v < cnt ? (uint32_t)v : cnt;
}

// what a pass over a pair's ops and columns hands to chk_finish
struct ChkTotals {
    uint32_t flags;        // steps 3, 5 and 7
    uint32_t len;          // OPS_LEN
    uint32_t m_count;      // cig_range(.., true)'s count
    uint64_t cost;         // saturating
    AltSums  all, trimmed; // alt_sums over all ops / over cig_range(.., true)'s
    ChkStats stats;        // over chk_stat_range's ops
    uint64_t n_bad, first_bad;  // step 7; first_bad ~0ull: none
};

// step 8 for one of the two renderings: count ops with the sums s render.  The text entries' own checks, in their order: a pair
// without an op in its range (COLUMNS_ONLY: without a column) is not looked at; the windows; alt_fits.
template <bool COLUMNS_ONLY, class Window>
__host__ __device__ inline bool chk_rows_fail(bool trim, uint32_t count, const AltSums s, Window &&window) {
    if (count == 0u || (COLUMNS_ONLY && s.cols == 0ull)) return false;
    AltWindow w;
    return !window(trim, &w) || !alt_fits(s, w);
}

// steps 4, 6 and 8 to 10, and the eight words.  window(trim, &w) gives the pair's windows as the text entries compute them
// (alt_window / alt_pk_window); COLUMNS_ONLY: the packed text entry's rule -- a pair whose ops have no column is not checked.
template <bool COLUMNS_ONLY, class Window>
__host__ __device__ inline void chk_finish(const ChkRule &R, const ChkRec &rec, const ChkTotals &T, uint32_t q_len, uint32_t t_len,
                                           Window &&window, uint32_t *out) {
    uint32_t f = T.flags;
    if (T.all.q > q_len) f |= CHK_Q_OVER;
    if (T.all.q < q_len) f |= CHK_Q_UNDER;
    if (T.all.t > t_len) f |= CHK_T_OVER;
    if (T.all.t < t_len) f |= CHK_T_UNDER;
    if (chk_rows_fail<COLUMNS_ONLY>(false, T.len, T.all, window)) f |= CHK_NO_ROWS;
    if (chk_rows_fail<COLUMNS_ONLY>(true, T.m_count, T.trimmed, window)) f |= CHK_NO_ROWS_TRIMMED;
    if (R.global) {
        if (T.cost > rec.score) f |= CHK_COST_OVER;
        if (T.cost < rec.score) f |= CHK_COST_UNDER;
    }
    if (T.stats.align_len != rec.align_len) f |= CHK_STAT_ALIGN_LEN;
    if (T.stats.matches != rec.matches) f |= CHK_STAT_MATCHES;
    if (T.stats.gaps != rec.gaps) f |= CHK_STAT_GAPS;
    if (T.stats.gap_regions != rec.gap_regions) f |= CHK_STAT_GAP_REGIONS;
    out[CHK_W_FLAGS]     = f;
    out[CHK_W_COST]      = chk_sat32(T.cost);
    out[CHK_W_Q_USED]    = chk_sat32(T.all.q);
    out[CHK_W_T_USED]    = chk_sat32(T.all.t);
    out[CHK_W_N_BAD]     = chk_sat32(T.n_bad);
    out[CHK_W_FIRST_BAD] = T.first_bad == ~0ull ? CHK_NONE : (T.first_bad > 0xFFFFFFFEull ? 0xFFFFFFFEu : (uint32_t)T.first_bad);
    out[6] = out[7] = 0u;
}

// steps 1 and 2 for a pair that gets no further: the eight words
__host__ __device__ inline void chk_unread(bool ops_range, uint32_t *out) {
    out[0] = ops_range ? CHK_OPS_RANGE | CHK_NO_ROWS | CHK_NO_ROWS_TRIMMED : 0u;
    out[1] = out[2] = out[3] = out[4] = out[5] = out[6] = out[7] = 0u;
}

// step 2's condition (compared without a sum that could wrap)
__host__ __device__ inline bool chk_ops_range(uint64_t ops_off, uint32_t ops_len, uint64_t ops_cap) {
    return ops_len > ops_cap || ops_off > ops_cap - ops_len;
}

// a pair's status for the stages behind the check
__host__ __device__ inline int32_t chk_pass(int32_t status, uint32_t flags, uint32_t mask) {
    return status != 0 ? status : ((flags & mask) != 0u ? CHK_PAIR_FAILED : 0);
}

// the sequences' bases for step 7, one at a time (the host's readers; the kernels use the display-row kernels')
struct ChkByteSeq {
    const uint8_t *q, *t;
    __host__ __device__ uint32_t q1(uint64_t p) const { return q[p]; }
    __host__ __device__ uint32_t t1(uint64_t p) const { return t[p]; }
};
struct ChkPkSeq {
    const uint32_t *qw, *tw;
    uint32_t        q_len, t_len;
    bool            rc;
    __host__ __device__ uint32_t q1(uint64_t p) const { return alt_pk_letter(qw, q_len, rc, (uint32_t)p); }
    __host__ __device__ uint32_t t1(uint64_t p) const { return alt_pk_letter(tw, t_len, false, (uint32_t)p); }
};

// the whole rule for one OK pair whose ops lie in the op buffer, op by op and column by column (the host entries; the kernels do
// the same in rounds of 64 ops and end in the same chk_finish).  seq() gives the readers once step 5 has passed.
template <bool COLUMNS_ONLY, class Window, class MakeSeq>
__host__ __device__ inline void chk_pair(const ChkRule &R, const ChkRec &rec, const uint64_t *ops, uint32_t len, uint32_t q_len,
                                         uint32_t t_len, Window &&window, MakeSeq &&seq, uint32_t *out) {
    ChkTotals T = {};
    T.len       = len;
    T.first_bad = ~0ull;
    uint32_t m_first, s_first, s_count;
    cig_range(ops, len, true, &m_first, &T.m_count);
    chk_stat_range(len, m_first, T.m_count, &s_first, &s_count);
    if (T.m_count == 0u) T.flags |= CHK_NO_M;
    AltWindow w;
    const bool seq_ok = window(false, &w);
    if (!seq_ok) T.flags |= CHK_SEQ_RANGE;
    for (uint32_t k = 0; k < len; k++) {
        const uint64_t op = ops[k];
        T.flags |= chk_op_flags(op, k != 0u, k != 0u ? (uint32_t)(ops[k - 1u] >> 32) : 0u);
        T.cost = chk_sat_add(T.cost, chk_op_cost(op, R));
        if (k - s_first < s_count) chk_stat_add(&T.stats, op);  // (unsigned: k >= s_first too)
        if (k - m_first < T.m_count) alt_add(&T.trimmed, op);
        if (seq_ok && chk_compares(op)) {
            const uint32_t v = chk_valid((uint32_t)op, T.all.q, T.all.t, q_len, t_len);
            if (v != 0u) {
                const auto S = seq();
                const bool m = cig_is_m(op);
                for (uint32_t c = 0; c < v; c++) {
                    const bool differ = S.q1(T.all.q + c) != S.t1(T.all.t + c);
                    if (differ == m) {
                        T.flags |= m ? CHK_M_DIFFERS : CHK_X_EQUAL;
                        if (T.n_bad++ == 0ull) T.first_bad = T.all.cols + c;
                    }
                }
            }
        }
        alt_add(&T.all, op);
    }
    chk_finish<COLUMNS_ONLY>(R, rec, T, q_len, t_len, window, out);
}

}  // namespace wfa
