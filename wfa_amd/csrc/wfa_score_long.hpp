// wfa_score_long.hpp -- wfa_score_long_kernel: the score-only forward pass of GLOBAL pairs of ANY length (wfahip_score_batch,
// wfahip_score_matrix: the pairs wfa_score_kernel hands back for their length).
//
// The row loop is wfa_score_kernel's (wfa_score.hpp: the exact WF_NEXT of wfa.go:549-700 with its rejections, the seeds of
// initComponents, WF_EXTEND on 2-bit words, the termination test before reduce, wf-adaptive's reduce, max_score), with two changes:
//   * the ring rows hold 32-bit offsets (0 = absent), so a read may be as long as WFAHIP_MAX_SEQ_LEN: SCORE_DM M rows, two I,
//     two D, SCORE_RW diagonals each -- 12 KB per pair.  A band wider than SCORE_BAND is handed back (ST_REDO_BAND);
//   * the sequences are NOT resident.  They come 2-bit packed (wfahip_pack_pairs' layout: 16 bases per word, word-aligned, one pad
//     word) from global memory; each keeps a window of P.lds_seq_words words in LDS that follows the least advanced cell of the
//     row (checked every eighth score step; it only moves forward, by at least half its length).  WF_EXTEND reads a 16-base
//     group from the window when both its words are inside, and from global memory when not: results never depend on the
//     window's size or position, and a match run longer than the window simply finishes on global loads.
// A wave per pair, a lane per diagonal, tiles of 64 diagonals.  The pairs are a list: entry 2i / 2i + 1 of P.mx_seq name the query
// / the target of pair i ({word offset lo, hi, length, -} into P.mx_words; the query's .w is the pair's slot of P.score_out; the target's
// .w != 0: the query's offset counts from P.mx_rc_words instead -- wfahip_score_batch_packed_device's flagged queries).
// MATRIX: the pair is a cell of a tile (wfa_matrix.hpp) and the kernel takes the cells with a sequence flagged MXF_LONG only --
// the others belong to wfa_score_kernel<MATRIX>, launched over the same tile.
// A query flagged for its reverse complement (wfahip_score_batch_packed_rc, wfahip_score_matrix_rc) is read from words wfa_rc_words_kernel
// wrote before this launch: the list's entry names them, a matrix row's lie P.mx_rc_shift words behind the table entry's.
#pragma once
#include "wfa_score.hpp"

namespace wfa {

constexpr uint32_t SCORE_LONG_WINDOW = 256;  // default window: packed words per sequence (4 096 bases)
// LDS words of a pair: the two windows, the 8 + 2 + 2 rows of 32-bit offsets, the bands {lo, hi} of the M rows
__host__ __device__ inline uint32_t score_long_lds_words(uint32_t win_words) {
    return 2u * win_words + (SCORE_DM + 4u) * SCORE_RW + 2u * SCORE_DM;
}
// a window size the kernel takes: a multiple of four words (the rows behind the windows stay 16-byte aligned)
inline uint32_t score_long_window(int64_t v) { return (v >= 16 && v <= 4096 && v % 4 == 0) ? (uint32_t)v : SCORE_LONG_WINDOW; }

#ifdef WFA_SCORE_UNIT
// The reverse complements of the flagged long queries of a call (wfahip_score_batch_packed_rc, wfahip_score_matrix_rc), written once behind
// the uploaded words: the windows of wfa_score_long_kernel slide forward over global memory, and reading a sequence backwards through them is
// not worth it.  A workgroup per job; job i is jobs[2 i] = {source word offset lo, hi, length, -} and jobs[2 i + 1] = {destination word offset
// lo, hi, -, -}, both into `words`: (length + 15) / 16 words and a zero pad word go to the destination.
__global__ __launch_bounds__(256) void wfa_rc_words_kernel(const uint4 *jobs, uint32_t *words, uint32_t n_jobs) {
    const uint32_t i = blockIdx.x;
    if (i >= n_jobs) return;
    const uint4           s = jobs[2ull * i], d = jobs[2ull * i + 1ull];
    const uint32_t *const src = words + ((uint64_t)s.y << 32 | s.x);
    uint32_t *const       dst = words + ((uint64_t)d.y << 32 | d.x);
    const uint32_t        nw  = (s.z + 15u) >> 4;
    for (uint32_t j = threadIdx.x; j < nw; j += 256u) dst[j] = rc_word(src, s.z, j);
    if (threadIdx.x == 0) dst[nw] = 0u;
}

template <bool MATRIX = false>
__global__ __launch_bounds__(64) void wfa_score_long_kernel(const KParams P) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int       lane = (int)threadIdx.x;
    const uint32_t  W    = P.lds_seq_words;
    uint32_t *const lq   = lds;
    uint32_t *const lt   = lds + W;
    uint32_t *const ring = lds + 2u * W;
    int *const      band = reinterpret_cast<int *>(ring + (SCORE_DM + 4) * SCORE_RW);  // lo of M row slot i at [i], hi at [SCORE_DM + i]
    const auto      rowM = [&](uint32_t i) -> uint32_t * { return ring + (i & (uint32_t)(SCORE_DM - 1)) * SCORE_RW; };
    const auto      rowI = [&](uint32_t i) -> uint32_t * { return ring + (SCORE_DM + (i & 1u)) * SCORE_RW; };
    const auto      rowD = [&](uint32_t i) -> uint32_t * { return ring + (SCORE_DM + 2 + (i & 1u)) * SCORE_RW; };
    const auto      rfl  = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
    const auto      lds_sync = [] {  // what one lane stored, another lane reads: in order, and not from a stale register
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    constexpr int BIG = 0x3FFFFFFF;

    const uint32_t idx = blockIdx.x;
    if (idx >= P.chunk_n) return;
    uint4    qd, td;
    uint32_t slot;
    if constexpr (MATRIX) {
        mx_cell(P, idx, qd, td);
        slot = idx;
        const uint32_t f = qd.w | td.w;
        if ((f & MXF_LONG) == 0u) return;  // wfa_score_kernel<MATRIX>'s cell
        // (the order the kernels test a pair in; a long cell with a byte outside ACGT stays on the full path)
        const uint32_t st = (f & MXF_EMPTY) ? ST_EMPTY : (f & MXF_TOO_LONG) ? ST_TOO_LONG : (f & MXF_BYTES) ? ST_REDO_BYTES : ST_PENDING;
        if (st != ST_PENDING) {
            if (lane == 0) P.score_out[slot] = make_uint2(st, 0u);
            return;
        }
    } else {
        const uint4 a = P.mx_seq[2ull * idx], b = P.mx_seq[2ull * idx + 1ull];
        qd = make_uint4(rfl(a.x), rfl(a.y), rfl(a.z), rfl(a.w)), td = make_uint4(rfl(b.x), rfl(b.y), rfl(b.z), rfl(b.w));
        slot = qd.w;
    }
    const auto emit = [&](uint32_t st, uint32_t sc) {
        if (lane == 0) P.score_out[slot] = make_uint2(st, sc);
    };
    // (a flagged query row of the matrix: the words wfa_rc_words_kernel wrote; the list's entry of a flagged pair names them itself --
    // in P.mx_words, or, the pair's target entry carrying .w != 0, in P.mx_rc_words: wfahip_score_batch_packed_device, whose words
    // are the caller's and cannot be written behind)
    const uint32_t *const gq = ((!MATRIX && td.w != 0u) ? P.mx_rc_words : P.mx_words) + ((uint64_t)qd.y << 32 | qd.x) +
                               ((MATRIX && (qd.w & MXF_RC) != 0u) ? P.mx_rc_shift : 0ull);
    const uint32_t *const gt = P.mx_words + ((uint64_t)td.y << 32 | td.x);
    // (the select above is 20 bytes of scalar code; 44 more, run once per pair, put the row loop's instructions back where they lay in
    // their 64-byte lines before it existed -- 20 bytes off them 2e4 x 50 kbp pairs took 129.7 ms in place of 127.6: KERNELS.md 4s)
    if constexpr (!MATRIX) {
#pragma unroll
        for (int k = 0; k < 11; k++) asm volatile("s_nop 0");
    }
    const int      n = (int)qd.z, m = (int)td.z, Ak = m - n;
    const uint32_t nwq = (qd.z + 15u) >> 4, nwt = (td.z + 15u) >> 4;  // index of each sequence's pad word

    // ---- the windows: words [w0, w0 + W) of a sequence, zero past its pad word
    uint32_t   qw0 = 0u, tw0 = 0u;
    const auto fill = [&](const uint32_t *g, uint32_t *l, uint32_t w0, uint32_t nw) {
        for (uint32_t j = (uint32_t)lane; j < W; j += 64u) l[j] = (w0 + j <= nw) ? g[w0 + j] : 0u;
    };
    // 16 bases from base p on (p < length: word p / 16 + 1 is at most the pad word)
    const auto win16 = [&](const uint32_t *g, const uint32_t *l, uint32_t w0, int p) -> uint32_t {
        const uint32_t w = (uint32_t)p >> 4, r = w - w0;
        uint32_t       a, b;
        if (WFA_OFTEN(r < W - 1u))
            a = l[r], b = l[r + 1u];
        else
            a = g[w], b = g[w + 1u];
        return __funnelshift_r(a, b, (uint32_t)(p & 15) * 2u);
    };
    // longest common prefix of q[v:], t[h:], clamped to the sequence ends (SeqView<0>::lcp)
    const auto lcp = [&](int v, int h) -> int {
        const int rem = imin2(n - v, m - h);
        int       tot = 0;
        while (tot < rem) {
            const uint32_t x = win16(gq, lq, qw0, v + tot) ^ win16(gt, lt, tw0, h + tot);
            if (x) {
                tot += __builtin_ctz(x) >> 1;
                break;
            }
            tot += 16;
        }
        return imin2(tot, rem);
    };
    fill(gq, lq, 0u, nwq), fill(gt, lt, 0u, nwt);
    if (lane < SCORE_DM) band[lane] = BIG, band[SCORE_DM + lane] = -BIG;
    const bool first_match = ((gq[0] ^ gt[0]) & 3u) == 0u;  // initComponents: the first bases (wfa.go:143-184)
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
        uint32_t *const Mn = rowM(si), *const Mx = rowM(si - dx), *const Mo = rowM(si - doe);
        uint32_t *const In = rowI(si), *const Ie = rowI(si - 1u), *const Dn = rowD(si), *const De = rowD(si - 1u);
        // the new rows' slots start empty (a row of SCORE_RW words is one 16-byte store per lane)
        reinterpret_cast<uint4 *>(Mn)[lane] = make_uint4(0u, 0u, 0u, 0u);
        reinterpret_cast<uint4 *>(In)[lane] = make_uint4(0u, 0u, 0u, 0u);
        reinterpret_cast<uint4 *>(Dn)[lane] = make_uint4(0u, 0u, 0u, 0u);
        lds_sync();

        // ---- next + seeds + extend, tile by tile
        int  mlo = BIG, mhi = -BIG, mind = BIG, maxd = -BIG, minh = BIG, minv = BIG;
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
            // initComponents' seed of this score: global alignment seeds diagonal 0 only, offset 1, at score 0 when the first bases
            // agree and at score x when not (Set = last write wins: next()'s cell stays)
            if (seeded && k == 0 && nM == 0u && s == (first_match ? 0u : x)) nM = 1u;
            if (nM != 0u) {
                int h = (int)nM;
                const int v = h - k;
                if (v > 0 && v < n && h < m) h += lcp(v, h), nM = (uint32_t)h;  // WF_EXTEND (wfa.go:394-455)
                mlo = imin2(mlo, k), mhi = imax2(mhi, k);
                if (k == Ak && h >= m) term = true;  // wfa.go:235-239
                const int vv = h - k;
                if (!(vv < 0 || vv >= n || h >= m)) {  // wfa.go:474-494
                    const int dd = imax2(m - h, n - vv);
                    mind = imin2(mind, dd), maxd = imax2(maxd, dd);
                    minh = imin2(minh, h), minv = imin2(minv, vv);
                }
            }
            const uint32_t r = RI(k);
            Mn[r] = nM, In[r] = nI, Dn[r] = nD;
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
                    Mn[r] = 0u, In[r] = 0u, Dn[r] = 0u;
                }
            }
        }
        if (lane == 0) {
            const uint32_t sl = si & (uint32_t)(SCORE_DM - 1);
            band[sl] = nhi >= nlo ? nlo : BIG, band[SCORE_DM + sl] = nhi >= nlo ? nhi : -BIG;
        }
        lds_sync();
        // ---- the windows follow the least advanced cell of this row, 128 bases of slack behind it for the cells that older rows
        // still source (a cell outside a window reads global memory: where the windows are decides speed only)
        if ((si & 7u) == 7u) {
            minh = wave_min(minh), minv = wave_min(minv);
            if (minh != BIG) {
                const uint32_t wq = (uint32_t)imax2(minv - 128, 0) >> 4, wt = (uint32_t)imax2(minh - 128, 0) >> 4;
                const bool     mq = wq > qw0 + W / 2u, mt = wt > tw0 + W / 2u;
                if (WFA_RARE(mq || mt)) {
                    if (mq) qw0 = wq, fill(gq, lq, qw0, nwq);
                    if (mt) tw0 = wt, fill(gt, lt, tw0, nwt);
                    lds_sync();
                }
            }
        }
    }
}
#endif

}  // namespace wfa
