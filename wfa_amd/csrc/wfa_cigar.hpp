// wfa_cigar.hpp -- the text of a CIGAR: ONE source of the rendering rule for the kernels (wfa_cigar.hip: wfahip_cigar_text_device,
// wfahip_align_batch_text) and the host renderer (wfahip_cigar_text).
//
// The rule is AlignmentResult.CIGAR(onlyAlignedRegion) of the reference (wfa_cigar.go:217-255):
//   * an op word is letter << 32 | count (wfa_cigar.go:118-124); it renders as the decimal of the count -- a full u32, so one to ten
//     digits, no leading zero, a count of 0 as "0" -- followed by the byte op >> 32, verbatim, whatever byte it is;
//   * the ops render in the order the record indexes them (they are already reversed and merged);
//   * onlyAlignedRegion renders the ops from the first 'M' op to the last 'M' op, inclusive (trimOps); a pair without an 'M' op,
//     where the reference would panic, renders the empty string.
// Nothing here needs HIP: the header compiles as plain C++ (tests/cigar_host_test.cpp).
#pragma once
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace wfa {

constexpr uint32_t CIG_MAX_OP_BYTES = 11;  // ten digits and the letter

__host__ __device__ inline bool cig_is_m(uint64_t op) { return (uint32_t)(op >> 32) == (uint32_t)'M'; }

// decimal digits of a count, 1 .. 10, by compares (a division loop would be ten dependent multiplies for every op)
__host__ __device__ inline uint32_t cig_digits(uint32_t c) {
    return 1u + (c >= 10u) + (c >= 100u) + (c >= 1000u) + (c >= 10000u) + (c >= 100000u) + (c >= 1000000u) + (c >= 10000000u) +
           (c >= 100000000u) + (c >= 1000000000u);
}

// bytes of an op's text
__host__ __device__ inline uint32_t cig_op_bytes(uint64_t op) { return cig_digits((uint32_t)op) + 1u; }

// the text of one op at dst[0 .. cig_op_bytes(op)); returns that length.  Writes no byte beyond it.
__host__ __device__ inline uint32_t cig_render(uint64_t op, uint8_t *dst) {
    uint32_t       c  = (uint32_t)op;
    const uint32_t nd = cig_digits(c);
    dst[nd]           = (uint8_t)(op >> 32);
    for (uint32_t d = nd; d-- > 0u;) {
        dst[d] = (uint8_t)('0' + c % 10u);
        c /= 10u;
    }
    return nd + 1u;
}

// the ops of a pair that render: [*first, *first + *count) of its len ops -- all of them, or under only_aligned the first 'M' op to
// the last one (count 0 without one).  The kernels find the same range with ballots over cig_is_m.
__host__ __device__ inline void cig_range(const uint64_t *ops, uint32_t len, bool only_aligned, uint32_t *first, uint32_t *count) {
    uint32_t a = 0, b = len;
    if (only_aligned) {
        while (a < len && !cig_is_m(ops[a])) a++;
        while (b > a && !cig_is_m(ops[b - 1u])) b--;
    }
    *first = a, *count = b - a;
}

// bytes of the text of count ops
__host__ __device__ inline uint64_t cig_text_bytes(const uint64_t *ops, uint32_t count) {
    uint64_t s = 0;
    for (uint32_t k = 0; k < count; k++) s += cig_op_bytes(ops[k]);
    return s;
}

// the text of count ops at dst[0 .. cig_text_bytes(ops, count)); returns that length
__host__ __device__ inline uint64_t cig_text_write(const uint64_t *ops, uint32_t count, uint8_t *dst) {
    uint64_t s = 0;
    for (uint32_t k = 0; k < count; k++) s += cig_render(ops[k], dst + s);
    return s;
}

}  // namespace wfa
