// wfa_diff.hpp -- the difference string of an alignment (minimap2's cs tag, short form): ONE source of the rendering rule for the
// kernels (wfa_cigar.hip: wfahip_diff_text_device, wfahip_diff_text_packed_device) and the host renderers (wfahip_diff_text,
// wfahip_diff_text_packed).
//
// The target is the reference sequence of the string: from the target's window and the string the query's window is rebuilt exactly.
//   * an op word is letter << 32 | count; its text is
//         'M'       ':' and the decimal of count (wfa_cigar.hpp's u32 decimal)      reads no base
//         'X'       per column '*', lc(target byte), lc(query byte)                  3 count bytes
//         'I'       '-' and lc of the count target bytes                            1 + count bytes
//         'D' 'H'   '+' and lc of the count query bytes                             1 + count bytes
//     an op of any other letter and an op of count 0 render nothing; bases are consumed exactly as alt_kind (wfa_altext.hpp) says;
//     lc(b) is b + 32 for 'A' <= b <= 'Z', every other byte verbatim.  Ops are taken at face value: an 'M' op is never compared with
//     the sequences, neighbouring ops of one letter are not merged;
//   * which ops render, over which windows, and when a pair is invalid are the display rows' (wfa_altext.hpp, wfa_altext_pk.hpp):
//     cig_range, alt_window / alt_pk_window and alt_fits decide, this header adds only the bytes of the text as a fourth 64-bit sum
//     (one 'X' op may render 3 x 0xFFFFFFFF bytes);
//   * packed input: alt_pk_letter / alt_pk_letters4 give the letters ("ACTG"[code], a flagged query reverse-complemented as it is
//     read), lower-cased here like any other byte.
// Nothing here needs HIP: the header compiles as plain C++ (tests/diff_host_test.cpp).
#pragma once
#include <stdint.h>

#include "wfa_altext_pk.hpp"

namespace wfa {

constexpr uint8_t  DIFF_MATCH = ':', DIFF_SUB = '*', DIFF_QUERY_ONLY = '+', DIFF_TARGET_ONLY = '-';
constexpr uint32_t DIFF_LANE_BYTES = 16;  // the write kernel: an op whose text is at most this long is rendered by its own lane

__host__ __device__ inline uint32_t diff_lc(uint32_t b) { return b - (uint32_t)'A' <= (uint32_t)('Z' - 'A') ? b + 32u : b; }

// diff_lc of the four bytes of v at once.  Bit 7 of a byte of ge / gt: its low seven bits are >= 'A' / > 'Z'; a byte with bit 7 set
// is no letter.  0x80 >> 2 is the 32 to add, and 'Z' + 32 carries into no neighbour.
__host__ __device__ inline uint32_t diff_lc4(uint32_t v) {
    const uint32_t low = v & 0x7F7F7F7Fu, ge = low + 0x3F3F3F3Fu, gt = low + 0x25252525u;
    return v + ((ge & ~gt & ~v & 0x80808080u) >> 2);
}

// the first byte of a gap's text: alt_kind ALT_T (an 'I' op, bases the target alone has) or ALT_Q ('D', 'H': the query alone)
__host__ __device__ inline uint8_t diff_gap_sign(uint32_t kind) { return kind == ALT_T ? DIFF_TARGET_ONLY : DIFF_QUERY_ONLY; }

// bytes of an op's text
__host__ __device__ inline uint64_t diff_op_bytes(uint64_t op) {
    const uint32_t kind = alt_kind(op), n = alt_cols(op);
    if (n == 0u) return 0ull;
    if (kind != (ALT_Q | ALT_T)) return 1ull + n;
    return cig_is_m(op) ? 1ull + cig_digits(n) : 3ull * n;
}

// the rows' three sums of a run of ops and the bytes of its text
struct DiffSums {
    AltSums  a;
    uint64_t bytes;
};

__host__ __device__ inline void diff_add(DiffSums *s, uint64_t op) {
    alt_add(&s->a, op);
    s->bytes += diff_op_bytes(op);
}

__host__ __device__ inline DiffSums diff_sums(const uint64_t *ops, uint32_t count) {
    DiffSums s = {{0, 0, 0}, 0};
    for (uint32_t k = 0; k < count; k++) diff_add(&s, ops[k]);
    return s;
}

// byte x < diff_op_bytes(op) of the text of an 'X' op or a gap of alt_kind kind whose first bases are qp and tp of the windows S
// reads: S.q1(p) / S.t1(p) give base p of the query's / target's window.  (The kernel's sweep over a long op; an 'M' op is short.)
template <class Seq>
__host__ __device__ inline uint32_t diff_op_byte(uint32_t kind, const Seq &S, uint64_t qp, uint64_t tp, uint64_t x) {
    if (kind == (ALT_Q | ALT_T)) {
        const uint64_t c = x / 3u;
        const uint32_t r = (uint32_t)(x - 3u * c);
        return r == 0u ? DIFF_SUB : diff_lc(r == 1u ? S.t1(tp + c) : S.q1(qp + c));
    }
    if (x == 0u) return diff_gap_sign(kind);
    return diff_lc(kind == ALT_T ? S.t1(tp + x - 1u) : S.q1(qp + x - 1u));
}

// the text of one op at dst[0 .. diff_op_bytes(op)); returns that length.  S.q4(p) / S.t4(p) give the bases p .. p + 3 of a window,
// base p + j in bits 8 j .., and are asked only for four bases of ONE op.  Writes no byte beyond the text; reads no base the op does
// not consume, an 'M' op none.
template <class Seq>
__host__ __device__ inline uint64_t diff_render(uint64_t op, const Seq &S, uint64_t qp, uint64_t tp, uint8_t *dst) {
    const uint32_t kind = alt_kind(op), n = alt_cols(op);
    if (n == 0u) return 0ull;
    if (kind == (ALT_Q | ALT_T)) {
        if (cig_is_m(op)) {
            const uint32_t nd = cig_digits(n);
            uint32_t       c  = n;
            dst[0]            = DIFF_MATCH;
            for (uint32_t d = nd; d > 0u; d--) {
                dst[d] = (uint8_t)('0' + c % 10u);
                c /= 10u;
            }
            return 1ull + nd;
        }
        for (uint32_t x = 0; x < n; x++) {
            dst[3ull * x]      = DIFF_SUB;
            dst[3ull * x + 1u] = (uint8_t)diff_lc(S.t1(tp + x));
            dst[3ull * x + 2u] = (uint8_t)diff_lc(S.q1(qp + x));
        }
        return 3ull * n;
    }
    const bool target = kind == ALT_T;
    dst[0]            = diff_gap_sign(kind);
    uint32_t x        = 0;
    for (; n - x >= 4u; x += 4u) {
        const uint32_t v = diff_lc4(target ? S.t4(tp + x) : S.q4(qp + x));
        for (uint32_t j = 0; j < 4u; j++) dst[1ull + x + j] = (uint8_t)(v >> (8u * j));
    }
    for (; x < n; x++) dst[1ull + x] = (uint8_t)diff_lc(target ? S.t1(tp + x) : S.q1(qp + x));
    return 1ull + n;
}

// the text of count ops at dst[0 .. diff_sums(ops, count).bytes), from the windows' first bases; returns that length
template <class Seq>
__host__ __device__ inline uint64_t diff_write(const uint64_t *ops, uint32_t count, const Seq &S, uint8_t *dst) {
    uint64_t at = 0, qp = 0, tp = 0;
    for (uint32_t k = 0; k < count; k++) {
        const uint64_t op   = ops[k];
        const uint32_t kind = alt_kind(op), n = alt_cols(op);
        at += diff_render(op, S, qp, tp, dst + at);
        if (kind & ALT_Q) qp += n;
        if (kind & ALT_T) tp += n;
    }
    return at;
}

// the host renderers' readers (the kernels' are wfa_cigar.hip's AltByteSeq / AltPkSeq): the windows' first bytes in a blob ...
struct DiffByteSeq {
    const uint8_t *qs, *ts;
    __host__ __device__ static uint32_t load4(const uint8_t *p) {
        uint32_t v;
        __builtin_memcpy(&v, p, 4);
        return v;
    }
    __host__ __device__ uint32_t q4(uint64_t p) const { return load4(qs + p); }
    __host__ __device__ uint32_t t4(uint64_t p) const { return load4(ts + p); }
    __host__ __device__ uint32_t q1(uint64_t p) const { return qs[p]; }
    __host__ __device__ uint32_t t1(uint64_t p) const { return ts[p]; }
};

// ... and the sequences' words with the windows' first bases (alt_pk_window's q_at / t_at)
struct DiffPkSeq {
    const uint32_t *qw, *tw;
    uint32_t        q_len, t_len, q_at, t_at;
    bool            rc;
    __host__ __device__ uint32_t q4(uint64_t p) const { return alt_pk_letters4(qw, q_len, rc, q_at + (uint32_t)p); }
    __host__ __device__ uint32_t t4(uint64_t p) const { return alt_pk_letters4(tw, t_len, false, t_at + (uint32_t)p); }
    __host__ __device__ uint32_t q1(uint64_t p) const { return alt_pk_letter(qw, q_len, rc, q_at + (uint32_t)p); }
    __host__ __device__ uint32_t t1(uint64_t p) const { return alt_pk_letter(tw, t_len, false, t_at + (uint32_t)p); }
};

}  // namespace wfa
