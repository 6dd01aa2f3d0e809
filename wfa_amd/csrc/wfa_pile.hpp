// wfa_pile.hpp -- the pileup of a batch's alignments over the target's storage: ONE source of the counting rule for the kernels
// (wfa_cigar.hip: wfahip_pileup_device, wfahip_pileup_packed_device) and the host entries (wfahip_pileup, wfahip_pileup_packed).
//
// Every product before this one is per PAIR; this one is per TARGET BASE.  A pileup is PILE_WORDS = 8 u32 counters for every base of
// a window [at, at + n) of the target's storage -- the byte index into the blob, or for packed words the base index 16 * woff + p --
// and every alignment of a batch adds to the counters of the bases it covers:
//   * an op word is letter << 32 | count.  With qs / ts the bases the ops before it consumed inside the pair's windows and T0 the
//     coordinate of the target window's first base:
//         'M' 'X'   column c: base T0 + ts + c gets + 1 in the word of query base qs + c -- A, C, T, G by the packer's code
//                   (byte >> 1) & 3 of a byte among ACGTacgt, OTHER for every other byte (packed input has none).  Ops are taken at
//                   face value: an 'M' column is not compared with the target, as in the difference string (wfa_diff.hpp)
//         'I'       column c: base T0 + ts + c gets + 1 in GAP (the query has no base there)
//         'D'       count > 0: ONE add of 1 to EXTRA and one of count to EXTRA_BASES at base T0 + max(ts, 1) - 1: the run of
//                   query-only bases hangs on the target base before it, a run in front of the window's first base on base 0;
//                   nothing when the target's window is empty
//         'H', any other letter, count 0: nothing ('H' consumes query bases, as in the display rows)
//   * an add happens only where the base lies in the pileup's window; adds are u32 and wrap; they commute, so the counters do not
//     depend on the order of pairs, threads or waves;
//   * which ops count, over which windows, and when a pair is invalid are the display rows' (wfa_altext.hpp, wfa_altext_pk.hpp):
//     cig_range, alt_window / alt_pk_window and alt_fits decide.  The target's bases are never read, the query's only under an 'M' or
//     'X' column inside the pileup's window;
//   * packed input: pile_pk_code gives the code straight from the words (base p of a flagged query is code ^ 2 of forward base
//     len - 1 - p); no letter is made.
// Nothing here needs HIP: the header compiles as plain C++ (tests/pile_host_test.cpp).
#pragma once
#include <stdint.h>

#include "wfa_altext_pk.hpp"

namespace wfa {

constexpr uint32_t PILE_WORDS = 8;
enum : uint32_t { PILE_W_A = 0, PILE_W_C, PILE_W_T, PILE_W_G, PILE_W_OTHER, PILE_W_GAP, PILE_W_EXTRA, PILE_W_EXTRA_BASES };
constexpr uint64_t PILE_MAX_N = (1ull << 61) / PILE_WORDS;  // bases of a window: its counters' bytes stay below 2^63

// the counter word of a query byte: the packer's code for ACGTacgt, OTHER for everything else
__host__ __device__ inline uint32_t pile_word_of_byte(uint32_t b) {
    const uint32_t u = b & 0xDFu;  // (upper case of a letter; no other byte becomes one of the four)
    return (u == 'A' || u == 'C' || u == 'G' || u == 'T') ? (b >> 1) & 3u : PILE_W_OTHER;
}

// the code of base p < len of the sequence packed at w, forward or (rc) reverse-complemented: alt_pk_letter without the letter.
// Reads one data word.
__host__ __device__ inline uint32_t pile_pk_code(const uint32_t *w, uint32_t len, bool rc, uint32_t p) {
    const uint32_t f = rc ? len - 1u - p : p;
    return ((w[f >> 4] >> (2u * (f & 15u))) & 3u) ^ (rc ? 2u : 0u);
}

// the pileup's window: n bases of the target's storage from base at on
struct PileWin {
    uint64_t at, n;
};

// base P lies in the window; *idx is then its place there (compared without a sum that could wrap)
__host__ __device__ inline bool pile_in(uint64_t P, const PileWin &W, uint64_t *idx) {
    *idx = P - W.at;
    return P >= W.at && *idx < W.n;
}

// of the n bases P0 .. P0 + n - 1 the ones [*lo, *hi) -- counted from P0 -- lie in the window; false: none does.  No loop over n:
// one op may hold 2^32 - 1 columns, and a kernel's round 64 such ops.
__host__ __device__ inline bool pile_clip(uint64_t P0, uint64_t n, const PileWin &W, uint64_t *lo, uint64_t *hi) {
    if (P0 >= W.at) {
        const uint64_t d = P0 - W.at;
        if (d >= W.n) return false;
        *lo = 0, *hi = n < W.n - d ? n : W.n - d;
    } else {
        const uint64_t d = W.at - P0;
        if (d >= n) return false;
        *lo = d, *hi = n - d < W.n ? n : d + W.n;  // (d + W.n < n here: no wrap)
    }
    return *lo < *hi;
}

// the base a 'D' run hangs on, ts target bases of the pair's window consumed before it
__host__ __device__ inline uint64_t pile_extra_base(uint64_t T0, uint64_t ts) { return T0 + (ts > 0u ? ts : 1u) - 1u; }

// the readers of the query's window: word(p) is the counter word of its base p ...
struct PileByteSeq {
    const uint8_t *qs;  // the window's first byte
    __host__ __device__ uint32_t word(uint64_t p) const { return pile_word_of_byte(qs[p]); }
};

// ... from bytes, and from the sequence's words with the window's first base (alt_pk_window's q_at)
struct PilePkSeq {
    const uint32_t *qw;
    uint32_t        q_len, q_at;
    bool            rc;
    __host__ __device__ uint32_t word(uint64_t p) const { return pile_pk_code(qw, q_len, rc, q_at + (uint32_t)p); }
};

// the adds of count ops of a pair that passed alt_fits: add(idx, word, v) is asked to add v to word `word` of the window's base
// idx.  T0 is the coordinate of the target window's first base, t_n the window's length.  Only the columns inside W are walked.
template <class Seq, class Add>
__host__ __device__ inline void pile_pair(const uint64_t *ops, uint32_t count, const Seq &S, uint64_t T0, uint32_t t_n, const PileWin &W,
                                          Add &&add) {
    uint64_t qs = 0, ts = 0;
    for (uint32_t k = 0; k < count; k++) {
        const uint64_t op   = ops[k];
        const uint32_t kind = alt_kind(op), n = alt_cols(op);
        if (kind & ALT_T) {
            uint64_t lo, hi;
            if (pile_clip(T0 + ts, n, W, &lo, &hi)) {
                const uint64_t idx0 = T0 + ts - W.at;  // (mod 2^64; idx0 + c is the place of column c wherever lo <= c < hi)
                for (uint64_t c = lo; c < hi; c++) add(idx0 + c, (kind & ALT_Q) ? S.word(qs + c) : (uint32_t)PILE_W_GAP, 1u);
            }
        } else if ((uint32_t)(op >> 32) == (uint32_t)'D' && n != 0u && t_n != 0u) {
            uint64_t idx;
            if (pile_in(pile_extra_base(T0, ts), W, &idx)) {
                add(idx, (uint32_t)PILE_W_EXTRA, 1u);
                add(idx, (uint32_t)PILE_W_EXTRA_BASES, n);
            }
        }
        if (kind & ALT_Q) qs += n;
        if (kind & ALT_T) ts += n;
    }
}

}  // namespace wfa
