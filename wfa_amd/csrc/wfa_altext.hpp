// wfa_altext.hpp -- the three display rows of an alignment: ONE source of the rendering rule for the kernels (wfa_cigar.hip:
// wfahip_alignment_text_device) and the host renderer (wfahip_alignment_text).
//
// The rule is AlignmentResult.AlignmentText(q, t, onlyAlignedRegion) of the reference (wfa_cigar.go:259-333): a query row, a row of
// bars and a target row, one column per aligned or gapped base.
//   * an op word is letter << 32 | count; its count columns are
//         'M'       query byte   '|'   target byte      consumes count query and count target bytes
//         'X'       query byte   ' '   target byte      consumes count query and count target bytes
//         'I'       '-'          ' '   target byte      consumes count target bytes
//         'D' 'H'   query byte   ' '   '-'              consumes count query bytes
//     any other letter gives no column and consumes nothing (the reference's switch has no default); sequence bytes are copied
//     verbatim, whatever they are;
//   * onlyAlignedRegion renders the ops cig_range (wfa_cigar.hpp) gives -- the first 'M' op to the last -- over the windows the
//     RECORD names, query bytes [QBEGIN - 1, QEND) and target bytes [TBEGIN - 1, TEND) as int32; the bases of the trimmed-away ops
//     are not summed.  Otherwise all ops render over the whole sequences;
//   * where the reference would index out of range the pair is invalid: alt_window and alt_fits say so before a byte is read.
// Nothing here needs HIP: the header compiles as plain C++ (tests/altext_host_test.cpp).
#pragma once
#include <stdint.h>

#include "wfa_cigar.hpp"

namespace wfa {

constexpr uint32_t ALT_Q = 1u, ALT_T = 2u;  // alt_kind's bits: the op's columns consume query / target bytes
constexpr uint8_t  ALT_GAP = '-', ALT_BAR = '|', ALT_BLANK = ' ';

// what an op's columns consume; 0: the op has no column
__host__ __device__ inline uint32_t alt_kind(uint64_t op) {
    switch ((uint32_t)(op >> 32)) {
    case 'M':
    case 'X': return ALT_Q | ALT_T;
    case 'I': return ALT_T;
    case 'D':
    case 'H': return ALT_Q;
    default: return 0u;
    }
}

// columns of an op
__host__ __device__ inline uint32_t alt_cols(uint64_t op) { return alt_kind(op) != 0u ? (uint32_t)op : 0u; }

// the byte of the middle row in an op's columns
__host__ __device__ inline uint8_t alt_a_byte(uint64_t op) { return cig_is_m(op) ? ALT_BAR : ALT_BLANK; }

// columns and bases of a run of ops, as 64-bit sums (one op holds a full u32)
struct AltSums {
    uint64_t cols, q, t;
};

__host__ __device__ inline void alt_add(AltSums *s, uint64_t op) {
    const uint32_t k = alt_kind(op), c = (uint32_t)op;
    if (k != 0u) s->cols += c;
    if (k & ALT_Q) s->q += c;
    if (k & ALT_T) s->t += c;
}

__host__ __device__ inline AltSums alt_sums(const uint64_t *ops, uint32_t count) {
    AltSums s = {0, 0, 0};
    for (uint32_t k = 0; k < count; k++) alt_add(&s, ops[k]);
    return s;
}

// the bytes of the blob a pair's rows read: q_n query bytes at q_at, t_n target bytes at t_at
struct AltWindow {
    uint64_t q_at, t_at;
    uint32_t q_n, t_n;
};

// one sequence's window; false where it leaves the sequence or the sequence leaves [0, blob_bytes)
__host__ __device__ inline bool alt_window_1(bool only_aligned, uint64_t blob_bytes, uint64_t off, uint32_t len, int32_t begin,
                                             int32_t end, uint64_t *at, uint32_t *n) {
    if (off > blob_bytes || len > blob_bytes - off) return false;  // (compared without a sum that could wrap)
    *at = off, *n = len;
    if (!only_aligned) return true;
    if (begin < 1 || begin - 1 > end || (uint32_t)end > len) return false;  // (end >= begin - 1 >= 0 where it is cast)
    *at = off + (uint32_t)(begin - 1), *n = (uint32_t)(end - (begin - 1));
    return true;
}

__host__ __device__ inline bool alt_window(bool only_aligned, uint64_t blob_bytes, uint64_t q_off, uint32_t q_len, uint64_t t_off,
                                           uint32_t t_len, int32_t qbegin, int32_t qend, int32_t tbegin, int32_t tend, AltWindow *w) {
    return alt_window_1(only_aligned, blob_bytes, q_off, q_len, qbegin, qend, &w->q_at, &w->q_n) &&
           alt_window_1(only_aligned, blob_bytes, t_off, t_len, tbegin, tend, &w->t_at, &w->t_n);
}

// the ops consume no base beyond the windows
__host__ __device__ inline bool alt_fits(const AltSums &s, const AltWindow &w) { return s.q <= w.q_n && s.t <= w.t_n; }

// the rows of count ops at q_row / a_row / t_row[0 .. alt_sums(ops, count).cols), from the windows' first bytes q and t; returns
// that length.  Reads alt_sums' q and t bytes, writes no byte beyond the rows.
__host__ __device__ inline uint64_t alt_rows_write(const uint64_t *ops, uint32_t count, const uint8_t *q, const uint8_t *t,
                                                   uint8_t *q_row, uint8_t *a_row, uint8_t *t_row) {
    uint64_t c = 0;
    for (uint32_t k = 0; k < count; k++) {
        const uint64_t op   = ops[k];
        const uint32_t kind = alt_kind(op), n = alt_cols(op);
        const uint8_t  a    = alt_a_byte(op);
        for (uint32_t x = 0; x < n; x++) {
            q_row[c + x] = (kind & ALT_Q) ? q[x] : ALT_GAP;
            a_row[c + x] = a;
            t_row[c + x] = (kind & ALT_T) ? t[x] : ALT_GAP;
        }
        if (kind & ALT_Q) q += n;
        if (kind & ALT_T) t += n;
        c += n;
    }
    return c;
}

}  // namespace wfa
