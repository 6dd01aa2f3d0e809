// wfa_score.hpp -- wfa_score_kernel: the score-only forward pass of GLOBAL alignments (wfahip_score_batch).
//
// The forward loop of AlignPointers (wfa.go:228-251) decides the score: the backtrace starts at M[s][Ak] of the terminating
// score s and never changes it (wfa.go:714).  A caller that wants the score only therefore needs none of what the full path
// keeps for the backtrace -- no arena rows, no decision bits, no pair_meta, no backtrace launch -- only the rows the next
// scores source: M[s-x], M[s-o-e], I[s-e], D[s-e].  Here they are BARE 16-bit offsets (0 = absent: an offset of a cell that
// exists is at least 1, wfa.go:143-184) in LDS rings indexed by diagonal modulo SCORE_RW:
//   * SCORE_DM M rows (slot = score index & 7: x/g and (o+e)/g up to 7 score steps back), two I and two D rows (e/g == 1: the
//     previous row); a new row never shares a slot with one of its sources, so nothing is updated in place;
//   * a wave per pair, a lane per diagonal, tiles of 64 diagonals (a row of a 1 kbp read at 5 % is one tile);
//   * per cell the exact WF_NEXT of wfa.go:549-700 without the tags (in score-only mode it does not matter which source wins),
//     rejections included (> m, offset - k > n), the seeds of initComponents (the first cell is always consumed as a match or
//     mismatch, wfa.go:143-184), WF_EXTEND on the 2-bit packed sequences (wfa.go:381-458);
//   * the termination test M[s][Ak] >= m after extend and before reduce (wfa.go:235-239), then wf-adaptive's reduce
//     (wfa.go:461-540) on the row as it stays in the ring;
//   * one {status, score} per pair goes out, nothing else.
// What it cannot hold -- a band wider than the ring (ST_REDO_BAND), a byte outside ACGT (ST_REDO_BYTES), a read longer than
// SCORE_MAX_LEN (ST_REDO_LDS) -- is handed back to the host, which aligns those pairs on the full path.
// MATRIX (wfahip_score_matrix): the workgroup's pair is a cell of a tile of the score matrix and its sequences come packed from the
// call's sequence table (wfa_matrix.hpp); the row loop is the same.
// STAGE_PACKED (wfahip_score_batch_packed): the pair comes from the list like the byte form's, but P.q_off / P.t_off count words of
// P.mx_words, which the caller packed: the words are copied into LDS as the matrix form copies them -- no byte load, no packing, no
// ACGT test.
#pragma once
#include "wfa_device.hpp"
#include "wfa_matrix.hpp"

namespace wfa {

constexpr uint32_t SCORE_MAX_LEN = 2047;  // 16-bit ring offsets (offsets overshoot to m + 1)
constexpr int      SCORE_RW = 256;        // halfwords of a ring row: diagonal k at slot k & 255
constexpr int      SCORE_DM = 8;          // M rows in the ring: DX and DOE up to SCORE_DM - 1
constexpr int      SCORE_BAND = SCORE_RW - 8;  // widest row the ring holds (its sources lie one diagonal beyond it on either side)
// LDS words of a pair: the two packed sequences, the 8 + 2 + 2 rows, the bands {lo, hi} of the M rows
__host__ __device__ inline uint32_t score_lds_words(uint32_t seq_words) {
    return ((2u * seq_words + 3u) & ~3u) + (SCORE_DM + 4u) * SCORE_RW / 2u + 2u * SCORE_DM;
}
// the penalty shapes the kernel takes: e / g == 1, x / g and (o+e) / g within the M ring
inline bool score_shape_ok(uint32_t dx, uint32_t doe, uint32_t de) {
    return de == 1u && dx >= 1u && doe >= 1u && dx < (uint32_t)SCORE_DM && doe < (uint32_t)SCORE_DM;
}

#ifdef WFA_SCORE_UNIT  // (the kernel lives in wfa_score.hip only; the host units take the constants)
template <int STAGE = STAGE_BYTES>
__global__ __launch_bounds__(64) void wfa_score_kernel(const KParams P) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int       lane = (int)threadIdx.x;
    const uint32_t  SW   = P.lds_seq_words;
    uint32_t *const lq   = lds;
    uint32_t *const lt   = lds + SW;
    uint16_t *const ring = reinterpret_cast<uint16_t *>(lds + ((2u * SW + 3u) & ~3u));
    int *const      band = reinterpret_cast<int *>(ring + (SCORE_DM + 4) * SCORE_RW);  // lo of M row slot i at [i], hi at [SCORE_DM + i]
    const auto      rowM = [&](uint32_t i) -> uint16_t * { return ring + (i & (uint32_t)(SCORE_DM - 1)) * SCORE_RW; };
    const auto      rowI = [&](uint32_t i) -> uint16_t * { return ring + (SCORE_DM + (i & 1u)) * SCORE_RW; };
    const auto      rowD = [&](uint32_t i) -> uint16_t * { return ring + (SCORE_DM + 2 + (i & 1u)) * SCORE_RW; };
    const auto      rfl  = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
    const auto      lds_sync = [] {  // what one lane stored, another lane reads: in order, and not from a stale register
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    constexpr int BIG = 0x3FFFFFFF;

    constexpr bool MATRIX = STAGE == STAGE_MATRIX;
    const uint32_t idx = blockIdx.x;
    if (idx >= P.chunk_n) return;
    const uint32_t pair = MATRIX ? idx : P.chunk_first + idx;  // (MATRIX: the cell's slot of the tile's output)
    const auto     emit = [&](uint32_t st, uint32_t sc) {
        if (lane == 0) P.score_out[pair] = make_uint2(st, sc);
    };
    uint32_t nq, mt;
    if constexpr (MATRIX) {
        uint4 qd, td;
        mx_cell(P, idx, qd, td);
        nq = qd.z, mt = td.z;
        const uint32_t st = mx_status(qd.w | td.w);  // (the table's flags: the tests below, made once per sequence)
        if (st != ST_PENDING) return emit(st, 0u);
        mx_stage<64>(P.mx_words, qd, lq, lane);
        mx_stage<64>(P.mx_words, td, lt, lane);
    } else {
    nq = rfl(P.q_len[pair]), mt = rfl(P.t_len[pair]);
    if (nq == 0u || mt == 0u) return emit(ST_EMPTY, 0u);                         // wfa.go:204-206
    if (nq > 0x1FFFFFFFu || mt > 0x1FFFFFFFu) return emit(ST_TOO_LONG, 0u);      // wfa.go:207-209
    const uint32_t ml = nq > mt ? nq : mt;
    if (ml > SCORE_MAX_LEN || (ml + 15u) / 16u + 1u > SW) return emit(ST_REDO_LDS, 0u);
    if constexpr (STAGE == STAGE_PACKED) {
        mx_stage<64>(P.mx_words, pk_entry(P.q_off, pair, nq, 0u, P.q_rc), lq, lane);
        mx_stage<64>(P.mx_words, pk_entry(P.t_off, pair, mt), lt, lane);
    } else {
        bool bad = stage_pack<64>(P.blob, P.q_off[pair], nq, lq, lane);
        bad |= stage_pack<64>(P.blob, P.t_off[pair], mt, lt, lane);
        if (__ballot(bad) != 0ull) return emit(ST_REDO_BYTES, 0u);  // a byte outside ACGT: the byte-compare path takes the pair
    }
    }
    const int n = (int)nq, m = (int)mt, Ak = m - n;
    SeqView<0> sv;
    sv.q = lq, sv.t = lt, sv.n = n, sv.m = m;
    if (lane < SCORE_DM) band[lane] = BIG, band[SCORE_DM + lane] = -BIG;
    lds_sync();

    const uint32_t x = P.x, g = P.g, dx = P.dx, doe = P.doe, maxs = P.max_score;
    const bool     adaptive = P.adaptive != 0u;
    const int      mdd = (int)P.max_dist_diff, minwf = (int)P.min_wf_len;
    const auto     blo = [&](uint32_t i) { return (int)rfl((uint32_t)band[i & (uint32_t)(SCORE_DM - 1)]); };
    const auto     bhi = [&](uint32_t i) { return (int)rfl((uint32_t)band[SCORE_DM + (i & (uint32_t)(SCORE_DM - 1))]); };
    const auto     RI  = [](int k) -> uint32_t { return (uint32_t)k & (uint32_t)(SCORE_RW - 1); };

    for (uint32_t si = 0;; si++) {
        const uint32_t s = si * g;
        if (maxs != 0u && s > maxs) return emit(ST_OVER_MAX, 0u);  // every row below s was computed and none terminated
        // ---- the range of next(s) (wfa.go:557-563) and of the seeds
        int lo = BIG, hi = -BIG;
        const bool hasX = si >= dx, hasO = si >= doe, hasE = si >= 1u;
        if (si != 0u) {
            const auto take = [&](int l, int h_) {
                if (h_ >= l) lo = imin2(lo, l - 1), hi = imax2(hi, h_ + 1);
            };
            if (hasX) take(blo(si - dx), bhi(si - dx));
            if (hasO) take(blo(si - doe), bhi(si - doe));
            take(blo(si - 1u), bhi(si - 1u));  // I[s-e], D[s-e] hold cells only where M[s-e] does
            lo = imax2(lo, -(n - 1)), hi = imin2(hi, m - 1);
        }
        const bool seeded = s == 0u || s == x;
        if (seeded) lo = imin2(lo, 0), hi = imax2(hi, 0);
        if (hi >= lo && hi - lo + 1 > SCORE_BAND) return emit(ST_REDO_BAND, 0u);
        uint16_t *const Mn = rowM(si), *const Mx = rowM(si - dx), *const Mo = rowM(si - doe);
        uint16_t *const In = rowI(si), *const Ie = rowI(si - 1u), *const Dn = rowD(si), *const De = rowD(si - 1u);
        // the new rows' slots start empty (a row of SCORE_RW halfwords is one 8-byte store per lane)
        reinterpret_cast<uint2 *>(Mn)[lane] = make_uint2(0u, 0u);
        reinterpret_cast<uint2 *>(In)[lane] = make_uint2(0u, 0u);
        reinterpret_cast<uint2 *>(Dn)[lane] = make_uint2(0u, 0u);
        lds_sync();

        // ---- next + seeds + extend, tile by tile
        int  mlo = BIG, mhi = -BIG, mind = BIG, maxd = -BIG;
        bool term = false;
        for (int t0 = lo; t0 <= hi; t0 += 64) {
            const int k = t0 + lane;
            if (k > hi) continue;
            uint32_t nM = 0u, nI = 0u, nD = 0u;
            if (si != 0u) {
                const uint32_t a0 = hasO ? Mo[RI(k - 1)] : 0u, c0 = hasO ? Mo[RI(k + 1)] : 0u;
                const uint32_t b0 = hasE ? Ie[RI(k - 1)] : 0u, d0 = hasE ? De[RI(k + 1)] : 0u;
                const uint32_t x0 = hasX ? Mx[RI(k)] : 0u;
                // rejections: > m (not >=) for I and X sources, offset - k > n for D and X sources (wfa.go:581-588,616-623,651-654)
                const uint32_t a = (int)a0 > m ? 0u : a0, b = (int)b0 > m ? 0u : b0;
                const uint32_t c = (int)c0 - k > n ? 0u : c0, d = (int)d0 - k > n ? 0u : d0;
                const uint32_t xx = ((int)x0 > m || (int)x0 - k > n) ? 0u : x0;
                const uint32_t mi = umax2(a, b);
                nI = mi + umin2(mi, 1u);
                nD = umax2(c, d);
                nM = umax2(umax2(nI, nD), xx + umin2(xx, 1u));
            }
            if (seeded && nM == 0u) {  // initComponents' seed of this score (Set = last write wins: next()'s cell stays)
                const uint32_t sw = seed_word<0>(sv, k, s, x, true);
                if (sw != 0u) nM = sw >> TAG_BITS;
            }
            if (nM != 0u) {
                int h = (int)nM;
                const int v = h - k;
                if (v > 0 && v < n && h < m) h += sv.lcp(v, h), nM = (uint32_t)h;  // WF_EXTEND (wfa.go:394-455)
                mlo = imin2(mlo, k), mhi = imax2(mhi, k);
                if (k == Ak && h >= m) term = true;  // wfa.go:235-239
                const int vv = h - k;
                if (!(vv < 0 || vv >= n || h >= m)) {  // wfa.go:474-494
                    const int dd = imax2(m - h, n - vv);
                    mind = imin2(mind, dd), maxd = imax2(maxd, dd);
                }
            }
            const uint32_t r = RI(k);
            Mn[r] = (uint16_t)nM, In[r] = (uint16_t)nI, Dn[r] = (uint16_t)nD;
        }
        lds_sync();
        if (__ballot(term) != 0ull) return emit(ST_OK, s);  // the termination test runs before reduce
        mlo = wave_min(mlo), mhi = wave_max(mhi), mind = wave_min(mind), maxd = wave_max(maxd);
        int nlo = mlo, nhi = mhi;
        if (adaptive && mhi >= mlo && (mhi - mlo + 1) >= minwf && mind != BIG && maxd - mind > mdd) {
            // ---- reduce (wfa.go:496-537): some distance fails
            const int thr = mind + mdd;
            int       first_ok = BIG, last_ok = -BIG;
            for (int t0 = mlo; t0 <= mhi; t0 += 64) {
                const int k = t0 + lane;
                if (k <= mhi) {
                    const int h = (int)Mn[RI(k)], v = h - k;
                    if (h != 0 && !(v < 0 || v >= n || h >= m) && imax2(m - h, n - v) <= thr) first_ok = imin2(first_ok, k), last_ok = imax2(last_ok, k);
                }
            }
            first_ok = wave_min(first_ok), last_ok = wave_max(last_ok);
            int lead = -BIG;  // _lo: one past the last valid entry before the first non-failing one (wfa.go:503-516)
            for (int t0 = mlo; t0 < first_ok && t0 <= mhi; t0 += 64) {
                const int k = t0 + lane;
                if (k < first_ok && k <= mhi) {
                    const int h = (int)Mn[RI(k)], v = h - k;
                    if (h != 0 && !(v < 0 || v >= n || h >= m)) lead = imax2(lead, k);
                }
            }
            lead = wave_max(lead);
            nlo  = lead != -BIG ? lead + 1 : mlo;
            nhi  = last_ok;  // wfa.go:517-524
            // wfa.go:526-535 deletes k outside [_lo, _hi] in M, I and D
            for (int t0 = mlo; t0 <= mhi; t0 += 64) {
                const int k = t0 + lane;
                if (k <= mhi && (k < nlo || k > nhi)) {
                    const uint32_t r = RI(k);
                    Mn[r] = 0, In[r] = 0, Dn[r] = 0;
                }
            }
        }
        if (lane == 0) {
            const uint32_t sl = si & (uint32_t)(SCORE_DM - 1);
            band[sl] = nhi >= nlo ? nlo : BIG, band[SCORE_DM + sl] = nhi >= nlo ? nhi : -BIG;
        }
        lds_sync();
    }
}
#endif

}  // namespace wfa
