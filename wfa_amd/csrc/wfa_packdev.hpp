// wfa_packdev.hpp -- 16 sequence bytes -> one 2-bit word: ONE source of the packing rule for the kernels of wfahip_pack_pairs_device
// (wfa_packdev.hip).  The words are those of the host packer (wfa_hostpack.hpp: pack8, pack_seq_fast), which
// tests/packdev_host_test.cpp and tests/test_packdev_host.py hold this function against.
//
// The rule (include/wfa_hip.h, "Pre-packed input"): the code of a base is (byte >> 1) & 3 -- A 0, C 1, T 2, G 3 --, base k of the
// piece goes to bits 2 k .. 2 k + 1, and the bits of the bases beyond the piece's last one are zero.  A byte is outside ACGT when it
// differs from the canonical letter of its own code (0x41 + 2 code, + 15 for T): lowercase letters, N and everything else.
// Nothing here needs HIP: the header compiles as plain C++.
#pragma once
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace wfa {

// Four bytes (the first one in the low bits of d) -> their four codes in the low eight bits; the first n (0 .. 4) bytes count, the
// others are taken as 'A' -- code 0, and never outside ACGT, whatever they hold.  *bad becomes non-zero when a byte that counts is
// outside ACGT and is left alone otherwise.
__host__ __device__ inline uint32_t pkd_pack4(uint32_t d, uint32_t n, uint32_t *bad) {
    const uint32_t m = n >= 4u ? 0xFFFFFFFFu : (1u << (8u * n)) - 1u;
    const uint32_t v = (d & m) | (0x41414141u & ~m);
    const uint32_t x = (v >> 1) & 0x03030303u;
    const uint32_t t = (x >> 1) & ~x & 0x01010101u;  // code 2 = 'T'
    *bad |= (0x41414141u + 2u * x + 15u * t) ^ v;
    const uint32_t y = (x | (x >> 6)) & 0x000F000Fu;
    return (y | (y >> 12)) & 0xFFu;
}

// Sixteen bytes as four dwords in address order (little endian) -> one word; the first n (1 .. 16) bytes are the piece, the bytes
// behind them neither reach the word nor count for *bad.
__host__ __device__ inline uint32_t pkd_word16(const uint32_t d[4], uint32_t n, uint32_t *bad) {
    uint32_t w = 0u;
    for (uint32_t k = 0; k < 4u; k++) w |= pkd_pack4(d[k], n > 4u * k ? n - 4u * k : 0u, bad) << (8u * k);
    return w;
}

}  // namespace wfa
