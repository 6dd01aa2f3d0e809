// wfa_altext_pk.hpp -- the display rows read from 2-bit packed words, both strands: ONE source of the decoding rule for the kernels
// (wfa_cigar.hip: wfahip_alignment_text_packed_device) and the host renderer (wfahip_alignment_text_packed).  The rows themselves
// are wfa_altext.hpp's: what differs is where a sequence's letters come from.
//   * the letter of a code is "ACTG"[code] -- A 0, C 1, T 2, G 3, the inverse of (ascii >> 1) & 3;
//   * base p of a forward sequence is bits 2 (p % 16) .. of word p / 16;
//   * base p of a flagged query of len bases is the complement (code ^ 2) of forward base len - 1 - p: the record's QBEGIN / QEND
//     and every op of a flagged pair are coordinates on that reverse complement, which exists nowhere as bytes.
// A sequence of len bases at word woff owns the words [woff, woff + alt_pk_words(len)): its data words and one pad word.  Nothing
// outside them is read, and no result depends on the bits of the last data word beyond the last base or on the pad word.
// Nothing here needs HIP: the header compiles as plain C++ (tests/altext_pk_host_test.cpp).
#pragma once
#include <stdint.h>

#include "wfa_altext.hpp"

namespace wfa {

constexpr uint32_t ALT_PK_LETTERS = 0x47544341u;  // "ACTG": byte code is the letter of that code

// wfahip_packed_words: the data words and the pad word
__host__ __device__ inline uint64_t alt_pk_words(uint32_t len) { return ((uint64_t)len + 15u) / 16u + 1u; }

// bits sh .. sh + 31 of hi:lo, sh < 32 (v_alignbit_b32 on the device)
__host__ __device__ inline uint32_t alt_pk_funnel(uint32_t lo, uint32_t hi, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, sh);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
#endif
}

// the letters of the four codes in bits 0 .. 7 of c, code j (bits 2 j ..) in byte j (one v_perm_b32 over ALT_PK_LETTERS on the device)
__host__ __device__ inline uint32_t alt_pk_letters_of(uint32_t c) {
    uint32_t sel = (c | (c << 12)) & 0x000F000Fu;  // codes 0, 1 in bits 0 .. 3, codes 2, 3 in bits 16 .. 19
    sel          = (sel | (sel << 6)) & 0x03030303u;  // a code to a byte
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(ALT_PK_LETTERS, ALT_PK_LETTERS, sel);
#else
    uint32_t v = 0;
    for (uint32_t j = 0; j < 4u; j++) v |= ((ALT_PK_LETTERS >> (8u * ((sel >> (8u * j)) & 3u))) & 0xFFu) << (8u * j);
    return v;
#endif
}

// the four bytes of v in reverse order
__host__ __device__ inline uint32_t alt_pk_bswap(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24); }

// the letter of base p < len of the sequence packed at w, forward or (rc) reverse-complemented.  Reads one data word.
__host__ __device__ inline uint8_t alt_pk_letter(const uint32_t *w, uint32_t len, bool rc, uint32_t p) {
    const uint32_t f    = rc ? len - 1u - p : p;
    const uint32_t code = ((w[f >> 4] >> (2u * (f & 15u))) & 3u) ^ (rc ? 2u : 0u);
    return (uint8_t)(ALT_PK_LETTERS >> (8u * code));
}

// the letters of the bases p .. p + 3 of that sequence, base p + j in bits 8 j ..; p + 4 <= len.  The four are forward bases f ..
// f + 3 (flagged: f = len - 4 - p, reversed and complemented), a funnel shift out of word f / 16 and the one behind it -- at most
// the pad word, whose bits are shifted out whenever it is reached, as are those of any word the four bases do not touch.
__host__ __device__ inline uint32_t alt_pk_letters4(const uint32_t *w, uint32_t len, bool rc, uint32_t p) {
    const uint32_t f = rc ? len - 4u - p : p, i = f >> 4;
    const uint32_t c = alt_pk_funnel(w[i], w[i + 1u], 2u * (f & 15u)) & 0xFFu;
    return rc ? alt_pk_bswap(alt_pk_letters_of(c ^ 0xAAu)) : alt_pk_letters_of(c);
}

// one sequence's window in BASES of the sequence, [*at, *at + *n): alt_window_1 with the packed sequence's words in place of the
// blob's bytes; false where the window leaves the sequence or the sequence's words leave [0, n_words)
__host__ __device__ inline bool alt_pk_window_1(bool only_aligned, uint64_t n_words, uint64_t woff, uint32_t len, int32_t begin,
                                                int32_t end, uint64_t *at, uint32_t *n) {
    if (woff > n_words || alt_pk_words(len) > n_words - woff) return false;  // (compared without a sum that could wrap)
    *at = 0u, *n = len;
    if (!only_aligned) return true;
    if (begin < 1 || begin - 1 > end || (uint32_t)end > len) return false;  // (end >= begin - 1 >= 0 where it is cast)
    *at = (uint32_t)(begin - 1), *n = (uint32_t)(end - (begin - 1));
    return true;
}

// both windows of a pair; w->q_at / t_at are base indices INSIDE the sequences (below 2^32), not addresses.  alt_fits applies.
__host__ __device__ inline bool alt_pk_window(bool only_aligned, uint64_t n_words, uint64_t q_woff, uint32_t q_len, uint64_t t_woff,
                                              uint32_t t_len, int32_t qbegin, int32_t qend, int32_t tbegin, int32_t tend, AltWindow *w) {
    return alt_pk_window_1(only_aligned, n_words, q_woff, q_len, qbegin, qend, &w->q_at, &w->q_n) &&
           alt_pk_window_1(only_aligned, n_words, t_woff, t_len, tbegin, tend, &w->t_at, &w->t_n);
}

// alt_rows_write over words: the query's bases from q_at on (reverse-complemented if q_rc), the target's from t_at on.  Four
// columns at a time inside an op, base by base at its end.  Writes no byte beyond the rows.
__host__ __device__ inline uint64_t alt_pk_rows_write(const uint64_t *ops, uint32_t count, const uint32_t *qw, uint32_t q_len, bool q_rc,
                                                      uint32_t q_at, const uint32_t *tw, uint32_t t_len, uint32_t t_at, uint8_t *q_row,
                                                      uint8_t *a_row, uint8_t *t_row) {
    uint64_t c = 0;
    for (uint32_t k = 0; k < count; k++) {
        const uint64_t op   = ops[k];
        const uint32_t kind = alt_kind(op), n = alt_cols(op);
        const uint8_t  a    = alt_a_byte(op);
        uint32_t       x    = 0;
        for (; n - x >= 4u; x += 4u) {
            const uint32_t qv = (kind & ALT_Q) ? alt_pk_letters4(qw, q_len, q_rc, q_at + x) : ALT_GAP * 0x01010101u;
            const uint32_t tv = (kind & ALT_T) ? alt_pk_letters4(tw, t_len, false, t_at + x) : ALT_GAP * 0x01010101u;
            for (uint32_t j = 0; j < 4u; j++) {
                q_row[c + x + j] = (uint8_t)(qv >> (8u * j));
                a_row[c + x + j] = a;
                t_row[c + x + j] = (uint8_t)(tv >> (8u * j));
            }
        }
        for (; x < n; x++) {
            q_row[c + x] = (kind & ALT_Q) ? alt_pk_letter(qw, q_len, q_rc, q_at + x) : ALT_GAP;
            a_row[c + x] = a;
            t_row[c + x] = (kind & ALT_T) ? alt_pk_letter(tw, t_len, false, t_at + x) : ALT_GAP;
        }
        if (kind & ALT_Q) q_at += n;
        if (kind & ALT_T) t_at += n;
        c += n;
    }
    return c;
}

}  // namespace wfa
