// wfa_rc.hpp -- the reverse complement of a 2-bit packed sequence, word by word: ONE source for the kernels' staging (mx_stage,
// wfa_rc_words_kernel, wfa_prepack_words_kernel), the host's gather of the pairs the kernels hand back and wfahip_revcomp_packed; and
// the addresses of the mirror from which the byte-reading passes of wfahip_align_batch_packed_rc take a flagged query (at the end).
//
// The packed code is (ascii >> 1) & 3 -- A 0, C 1, T 2, G 3 -- so the complement of a base is code ^ 2 and that of a word is
// word ^ 0xAAAAAAAA.  Base i of the result is base len - 1 - i of the source: the sixteen 2-bit groups of a word are reversed (a bit
// reversal, v_bfrev_b32 on the device, and a swap of adjacent bits to put each group's two bits back in order), the words are taken
// from the last one down, and -- the source's last word holding pad = 16 nw - len groups beyond its last base, which land at the LOW
// end of the first reversed word -- every result word is a funnel shift by 2 pad bits across two of them.
// Nothing here needs HIP: the header compiles as plain C++ (tests/rc_host_test.cpp).
#pragma once
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace wfa {

// the sixteen 2-bit groups of w in reverse order
__host__ __device__ inline uint32_t rc_rev2(uint32_t w) {
#if defined(__clang__)
    w = __builtin_bitreverse32(w);
#else
    w = (w >> 16) | (w << 16);
    w = ((w >> 8) & 0x00FF00FFu) | ((w & 0x00FF00FFu) << 8);
    w = ((w >> 4) & 0x0F0F0F0Fu) | ((w & 0x0F0F0F0Fu) << 4);
    w = ((w >> 2) & 0x33333333u) | ((w & 0x33333333u) << 2);
    w = ((w >> 1) & 0x55555555u) | ((w & 0x55555555u) << 1);
#endif
    return ((w >> 1) & 0x55555555u) | ((w & 0x55555555u) << 1);
}

// Word j (j < nw = (len + 15) / 16) of the reverse complement of the len >= 1 bases packed at src.  Reads src[nw - 1 - j] and, when the
// source's last word is not full and j + 1 < nw, src[nw - 2 - j]: never a word below src[0], never the pad word src[nw].  The bits of
// the source's last word beyond its last base are shifted out, whatever they hold; the bits of the result's last word beyond
// its last base are zero.
__host__ __device__ inline uint32_t rc_word(const uint32_t *src, uint32_t len, uint32_t j) {
    const uint32_t nw = (len + 15u) >> 4, sh = 2u * (16u * nw - len);
    const uint32_t a  = rc_rev2(src[nw - 1u - j]) ^ 0xAAAAAAAAu;
    if (sh == 0u) return a;
    const uint32_t b = j + 1u < nw ? rc_rev2(src[nw - 2u - j]) ^ 0xAAAAAAAAu : 0u;
    return a >> sh | b << (32u - sh);
}

// ---- the mirror of a packed call's byte blob (wfahip_align_batch_packed_rc).  The passes that read BYTES take a flagged query from
// an address of its own: behind the B = 16 n_words bytes the words stand for (and a gap) lies their mirror image, byte Mir(a) =
// TOP - a the COMPLEMENT of forward byte a, TOP = 2 B + 47.  The reverse complement of any (word offset, len) is then the len
// contiguous bytes from rc_mirror_off -- a substring of the mirror, for every length and every offset, so pairs that share a query
// under different lengths share mirror bytes and never disagree on one: a mirror byte is a function of ONE forward word.  The
// mirror of forward word w is the 16-byte aligned block at rc_mirror_block, holding rc_mirror_letters(word): one aligned 16-byte
// store per word.  The blob of a call with flags is rc_mirror_bytes long.
__host__ __device__ inline uint64_t rc_mirror_top(uint64_t n_words) { return 32u * n_words + 47u; }
__host__ __device__ inline uint64_t rc_mirror_bytes(uint64_t n_words) { return 32u * n_words + 96u; }
// byte address of the reverse complement of the len bases packed from word woff on
__host__ __device__ inline uint64_t rc_mirror_off(uint64_t top, uint64_t woff, uint32_t len) { return top + 1u - 16u * woff - len; }
// ... and back: the word offset of the forward sequence whose len-base reverse complement starts at mirror address off
__host__ __device__ inline uint64_t rc_mirror_word(uint64_t top, uint64_t off, uint32_t len) { return (top + 1u - off - len) >> 4; }
// where the 16 mirror bytes of forward word w start (16-byte aligned: TOP + 1 is a multiple of 16)
__host__ __device__ inline uint64_t rc_mirror_block(uint64_t top, uint64_t w) { return top - 15u - 16u * w; }
// the 16 letters of that block, in address order, four to a dword: the word's bases from the last one down, complemented
__host__ __device__ inline void rc_mirror_letters(uint32_t word, uint32_t o[4]) {
    const uint32_t w = rc_rev2(word) ^ 0xAAAAAAAAu;
    for (int d = 0; d < 4; d++) {
        uint32_t v = 0;
        for (int b = 0; b < 4; b++) v |= ((0x47544341u >> (8u * ((w >> (2 * (4 * d + b))) & 3u))) & 0xFFu) << (8 * b);  // "ACTG"[code]
        o[d] = v;
    }
}

}  // namespace wfa
