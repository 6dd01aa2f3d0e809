// wfa_matrix.hpp -- the prologue the score kernels run in their matrix instances (wfahip_score_matrix: every query against every
// target).  The host packs each of the n_q + n_t sequences ONCE into a table of 2-bit words and flags it once; a workgroup
// finds its cell in a rectangular tile, copies the two sequences' packed words into LDS (no byte loads, no packing per cell)
// and runs the row loop of the kernel it is an instance of, unchanged.
// The packed pair-list instances (wfahip_score_batch_packed) share the copy: their pairs come as a list of word offsets and lengths
// over words the CALLER packed (wfahip_pack_pairs' layout), tested per pair as the byte instances test theirs.
#pragma once
#include "wfa_common.hpp"
#include "wfa_rc.hpp"

namespace wfa {

// where a score kernel's prologue takes its pair from (template argument STAGE of wfa_score_kernel and the score instances of
// wfa_wide_kernel): bytes of the call's blob, 2-bit packed by the workgroup (stage_pack); a cell of a tile over the call's sequence
// table; a pair of the list P.q_off / q_len / t_off / t_len whose offsets count WORDS of P.mx_words
enum : int { STAGE_BYTES = 0, STAGE_MATRIX = 1, STAGE_PACKED = 2 };

// flags of a sequence of the table (KParams::mx_seq[i].w); a cell takes the status of its two sequences' flags, OR-ed, in the
// order the kernels test a pair: empty, too long, longer than the kernels take, a byte outside ACGT
enum : uint32_t { MXF_EMPTY = 1u, MXF_TOO_LONG = 2u, MXF_LONG = 4u, MXF_BYTES = 8u };
// ... and, in the descriptor a kernel stages from (never in the table): the cell or pair takes the REVERSE COMPLEMENT of this sequence
// (wfahip_score_matrix_rc, wfahip_score_batch_packed_rc: P.q_rc).  Not a status: mx_status does not look at it
constexpr uint32_t MXF_RC = 16u;

__host__ __device__ inline uint32_t mx_status(uint32_t f) {
    return (f & MXF_EMPTY) ? ST_EMPTY : (f & MXF_TOO_LONG) ? ST_TOO_LONG : (f & MXF_LONG) ? ST_REDO_LDS : (f & MXF_BYTES) ? ST_REDO_BYTES : ST_PENDING;
}

// the table entries of cell idx of the tile (wave-uniform: one scalar division per workgroup).  The reverse-complement flag belongs to
// the query ROW, not to the table entry: a table over the same arrays holds a sequence once, forward in its target role
__device__ inline void mx_cell(const KParams &P, uint32_t idx, uint4 &qd, uint4 &td) {
    const uint32_t r = idx / P.mx_cols, c = idx - r * P.mx_cols;
    const uint4    a = P.mx_seq[P.mx_r0 + r], b = P.mx_seq[P.mx_tbase + P.mx_c0 + c];
    const auto     rfl = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
    qd = make_uint4(rfl(a.x), rfl(a.y), rfl(a.z), rfl(a.w)), td = make_uint4(rfl(b.x), rfl(b.y), rfl(b.z), rfl(b.w));
    if (P.q_rc != nullptr && rfl(P.q_rc[P.mx_r0 + r]) != 0u) qd.w |= MXF_RC;
}
// entry of pair `pair` of a packed pair list (wave-uniform): {word offset lo, hi, length, 0 or MXF_RC}; rc: the list's flags (nullptr: none set)
// (shift = 4: the offsets count BYTES of the blob the words stand for, 16 to a word -- the full-alignment path, wfa_scale_offsets_kernel)
// (top != 0, the full-alignment path with flags, wfahip_align_batch_packed_rc: a flagged pair's offset is the mirror address of its
// reverse complement -- the entry names the forward words it was made from, wfa_rc.hpp)
__device__ inline uint4 pk_entry(const uint64_t *woff, uint32_t pair, uint32_t len, uint32_t shift = 0u, const uint8_t *rc = nullptr, uint64_t top = 0u) {
    uint64_t       o   = woff[pair] >> shift;
    const auto     rfl = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
    const uint32_t f   = (rc != nullptr && rfl(rc[pair]) != 0u) ? MXF_RC : 0u;
    if (WFA_RARE(f != 0u && top != 0u)) o = rc_mirror_word(top, woff[pair], len);
    return make_uint4(rfl((uint32_t)o), rfl((uint32_t)(o >> 32)), len, f);
}
// words 0 .. (len + 15) / 16 of a packed sequence (the last one its pad word) into LDS: stage_pack's layout.  (Caller-packed words:
// the pad word and the bits of the last word beyond the sequence may hold anything -- SeqView<0>::lcp clamps to the sequence ends,
// the seeds read bases inside them)
// d.w & MXF_RC (uniform over the workgroup): the words of the sequence's reverse complement instead, made from the same source words
// as they are copied (wfa_rc.hpp: two loads, a bit reversal and a funnel shift per word), and a zero pad word
template <int G>
__device__ inline void mx_stage(const uint32_t *words, const uint4 &d, uint32_t *dst, int tid) {
    const uint32_t *const src = words + ((uint64_t)d.y << 32 | d.x);
    const uint32_t        nw  = (d.z + 15u) >> 4;
    if (WFA_RARE((d.w & MXF_RC) != 0u)) {
        for (uint32_t j = (uint32_t)tid; j < nw; j += G) dst[j] = rc_word(src, d.z, j);
        if (tid == 0) dst[nw] = 0u;
        return;
    }
    for (uint32_t j = (uint32_t)tid; j <= nw; j += G) dst[j] = src[j];
}

}  // namespace wfa
