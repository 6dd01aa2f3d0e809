// wfa_score_dev.hpp -- the device-side routing of wfahip_score_batch_device: what score_batch_impl (wfa_entry.hip) does on the
// host with the sequences in its hands, done on the device for a batch that lives in HBM.  Nothing proportional to the batch
// crosses PCIe: the host fetches one block of SDC_WORDS counters per phase and decides from them.
//
//   wfa_score_plan_kernel   a thread per pair over the offset / length arrays: the bounds check of the host entries (a non-empty
//                           pair within WFAHIP_MAX_SEQ_LEN whose query or target leaves [0, blob_bytes)), the longest length, and
//                           score_long_plan's list -- the global pairs with a read beyond SCORE_MAX_LEN, in batch order, with the
//                           word offsets of their sequences in the packed buffer (wfahip_packed_words(len) each, query then target)
//   wfa_score_pack_kernel   2-bit packs the listed sequences from the caller's blob into that buffer: wfahip_pack_pairs' layout, byte
//                           for byte what pack_seq_fast writes on the host.  A workgroup per sequence, a lane per word: one aligned
//                           16-byte load (two when the sequence does not start on a 16-byte boundary: the second one hits the
//                           line the next lane has just fetched), one 4-byte store, a wave writing 64 consecutive words
//   wfa_score_list_kernel   the table wfa_score_long_kernel reads (KParams::mx_seq): two entries per listed pair WITHOUT a byte outside
//                           ACGT, in batch order; the others are marked ST_REDO_BYTES and stay on the full path, as on the host
//   wfa_score_redo_kernel   after the score kernels: the pairs they handed back (status >= ST_REDO_BYTES), in pair order, with their
//                           offsets and lengths in compact arrays align_device() takes as they are -- the offsets keep pointing into
//                           the caller's blob
//   wfa_score_finish_kernel {status, score} records -> the caller's d_status / d_score; the records of the full path's pairs -> the
//                           same (the full path ran under the call's max_score: its records say ST_OVER_MAX themselves)
//
// Lists in batch order come from a scan, not from a per-pair atomic: every selection is two launches over tiles of SD_TILE items --
// count (tile sums -> blk[]), then write (rank = blk[tile] + rank within the tile) -- with wfa_score_scan_kernel, one workgroup
// that turns the tile sums into exclusive prefixes and leaves the totals in the control words, between them.  No workgroup
// waits for another.
#pragma once
#include "wfa_common.hpp"
#include "wfa_score.hpp"

namespace wfa {

constexpr uint32_t SD_BLOCK = 256, SD_ITEMS = 4, SD_TILE = SD_BLOCK * SD_ITEMS;
constexpr uint32_t SD_MAX_SEQ_LEN = 0x1FFFFFFFu;  // WFAHIP_MAX_SEQ_LEN (wfa.go:186-193), as the kernels spell it
// the control words (uint64 each): one 64-byte fetch shows the host all of them
enum { SDC_BOUNDS = 0, SDC_MAX_LEN, SDC_N_LONG, SDC_N_WORDS, SDC_N_LISTED, SDC_N_REDO, SDC_REDO_SUM, SDC_REDO_MAX, SDC_WORDS };
// (wfahip_score_batch_packed_device lists nothing in a second step: that word carries "a flag is set"; its SDC_N_WORDS counts the words of
// the flagged long queries' reverse complements, its SDC_REDO_SUM the words of the pairs of the full path)
enum { SDC_ANY_RC = SDC_N_LISTED };
enum { SDK_PLAN_COUNT = 0, SDK_PLAN_WRITE, SDK_SCAN, SDK_PACK, SDK_LIST_COUNT, SDK_LIST_WRITE, SDK_REDO_COUNT, SDK_REDO_WRITE, SDK_FINISH,
       // wfahip_score_batch_packed_device (at the end of this header)
       SDK_PK_PLAN_COUNT, SDK_PK_PLAN_WRITE, SDK_PK_RCQ, SDK_PK_REDO_COUNT, SDK_PK_REDO_WRITE, SDK_PK_GATHER,
       // wfahip_select_pairs_device
       SDK_SELECT_COUNT, SDK_SELECT_WRITE };

struct SDSum {
    unsigned long long cnt, wt;  // selected items of a tile; their weight (plan: packed words, redo: bases)
};

struct SDParams {
    // the caller's batch (never written)
    const uint8_t  *blob;
    uint64_t        blob_bytes;
    const uint64_t *q_off, *t_off;
    const uint32_t *q_len, *t_len;
    uint64_t        n;          // items of this launch: pairs (plan, redo, finish), listed long pairs (pack, list), tiles (scan)
    uint32_t        want_long;  // plan: 1 = list the long pairs (a global call on a shape wfa_score_kernel takes)
    uint32_t        all;        // redo: 1 = every pair (a penalty shape without an instance)
    uint32_t        c_cnt, c_wt;  // scan: the control words that take the totals
    unsigned long long *ctl;    // [SDC_WORDS]
    SDSum          *blk;        // per tile: its sums, then (after the scan) the sums of the tiles before it
    // the long pairs, in batch order
    uint32_t       *l_id;       // pair index
    uint64_t       *l_qw, *l_tw;  // word offsets of query and target in `words`
    uint32_t       *l_bad;      // 1: a byte outside ACGT
    uint32_t       *words;      // the packed buffer (ctx->mx_words)
    uint4          *table;      // KParams::mx_seq of wfa_score_long_kernel
    uint2          *score_out;  // {status, score} per pair (KParams::score_out)
    // the pairs of the full path, in pair order
    uint32_t       *r_id;
    uint64_t       *r_qoff, *r_toff;
    uint32_t       *r_qlen, *r_tlen;
    // finish
    int32_t        *d_status;
    uint32_t       *d_score;
    const uint32_t *rec;        // nullptr: from score_out; else the records of pairs r_id[first ..] of the full path
    uint64_t        first;
    uint32_t        max_score;  // (the call's bound; the full path gets it through the context)
    // wfahip_score_batch_packed_device: q_off / t_off count words of pk_words
    const uint32_t *pk_words;   // the caller's 2-bit words (never written)
    uint64_t        n_words;
    const uint8_t  *q_rc;       // a flag per pair, nullptr = none set (wfahip_select_pairs_device: the flags to compact)
    uint32_t       *rc_words;   // the reverse complements of the flagged long queries (KParams::mx_rc_words)
    uint32_t       *g_words;    // the words of the pairs of the full path, as wfahip_pack_pairs lays them out; r_qoff / r_toff count its words
    uint8_t        *r_rc;       // (the full path gets no flags: the gather has applied them.  wfahip_select_pairs_device: the compacted flags)
    // wfahip_select_pairs_device: the statuses it selects by; its outputs are r_id (may be nullptr), r_qoff, r_toff, r_qlen, r_tlen, r_rc
    const int32_t  *sel_status;
};

#ifdef WFA_SCORE_UNIT
__device__ inline uint64_t sd_words(uint32_t len) { return ((uint64_t)len + 15u) / 16u + 1u; }  // wfahip_packed_words
__device__ inline bool     sd_valid(uint32_t ql, uint32_t tl) { return ql != 0u && tl != 0u && ql <= SD_MAX_SEQ_LEN && tl <= SD_MAX_SEQ_LEN; }

// exclusive prefix of (c, w) over the SD_BLOCK threads of a workgroup, and the workgroup's totals
__device__ inline void sd_block_scan(unsigned long long c, unsigned long long w, unsigned long long &ec, unsigned long long &ew,
                                     unsigned long long &tc, unsigned long long &tw) {
    __shared__ unsigned long long s_c[SD_BLOCK / 64], s_w[SD_BLOCK / 64];
    const uint32_t     lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    unsigned long long ic = c, iw = w;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const unsigned long long a = __shfl_up(ic, d, 64), b = __shfl_up(iw, d, 64);
        if (lane >= d) ic += a, iw += b;
    }
    if (lane == 63u) s_c[wv] = ic, s_w[wv] = iw;
    __syncthreads();
    ec = ic - c, ew = iw - w, tc = 0, tw = 0;
#pragma unroll
    for (uint32_t v = 0; v < SD_BLOCK / 64; v++) {
        if (v < wv) ec += s_c[v], ew += s_w[v];
        tc += s_c[v], tw += s_w[v];
    }
    __syncthreads();  // (the next call writes s_c / s_w again)
}

// One tile of a selection.  pred(i, sel, wt): is item i selected, and with which weight; emit(i, rank, woff): item i is the
// rank-th selected one of the launch and the weights of those before it sum to woff.  WRITE = false: the tile's sums only.
template <bool WRITE, class Pred, class Emit>
__device__ inline void sd_select(const SDParams &S, Pred pred, Emit emit) {
    const uint64_t     i0 = ((uint64_t)blockIdx.x * SD_BLOCK + threadIdx.x) * SD_ITEMS;
    uint32_t           sel[SD_ITEMS];
    uint64_t           wt[SD_ITEMS];
    unsigned long long c = 0, w = 0;
#pragma unroll
    for (uint32_t k = 0; k < SD_ITEMS; k++) {
        sel[k] = 0u, wt[k] = 0ull;
        if (i0 + k < S.n) pred(i0 + k, sel[k], wt[k]);
        if (!sel[k]) wt[k] = 0ull;
        c += sel[k], w += wt[k];
    }
    unsigned long long ec, ew, tc, tw;
    sd_block_scan(c, w, ec, ew, tc, tw);
    if constexpr (!WRITE) {
        if (threadIdx.x == 0) S.blk[blockIdx.x] = SDSum{tc, tw};
    } else {
        const SDSum base = S.blk[blockIdx.x];
        uint64_t    r = base.cnt + ec, wo = base.wt + ew;
#pragma unroll
        for (uint32_t k = 0; k < SD_ITEMS; k++)
            if (sel[k]) emit(i0 + k, r, wo), r++, wo += wt[k];
    }
}

// tile sums -> exclusive prefixes, in place; the totals -> ctl[c_cnt], ctl[c_wt].  One workgroup; S.n = tiles
__global__ __launch_bounds__(SD_BLOCK) void wfa_score_scan_kernel(const SDParams S) {
    unsigned long long cc = 0, cw = 0;
    for (uint64_t b0 = 0; b0 < S.n; b0 += SD_BLOCK) {
        const uint64_t j = b0 + threadIdx.x;
        const SDSum    v = j < S.n ? S.blk[j] : SDSum{0ull, 0ull};
        unsigned long long ec, ew, tc, tw;
        sd_block_scan(v.cnt, v.wt, ec, ew, tc, tw);
        if (j < S.n) S.blk[j] = SDSum{cc + ec, cw + ew};
        cc += tc, cw += tw;
    }
    if (threadIdx.x == 0) S.ctl[S.c_cnt] = cc, S.ctl[S.c_wt] = cw;
}

template <bool WRITE>
__global__ __launch_bounds__(SD_BLOCK) void wfa_score_plan_kernel(const SDParams S) {
    uint32_t mx = 0u, oob = 0u;
    sd_select<WRITE>(
        S,
        [&](uint64_t i, uint32_t &sel, uint64_t &wt) {
            const uint32_t ql = S.q_len[i], tl = S.t_len[i];
            if (!sd_valid(ql, tl)) return;  // (empty or too long: never read, so never checked -- the host entries' rule)
            if constexpr (!WRITE) {
                const uint64_t qo = S.q_off[i], to = S.t_off[i], bb = S.blob_bytes;
                // (written so that a hostile 64-bit offset cannot wrap the sum around)
                if (qo > bb || ql > bb - qo || to > bb || tl > bb - to) oob = 1u;
                mx = umax2(mx, umax2(ql, tl));
            }
            if (S.want_long != 0u && umax2(ql, tl) > SCORE_MAX_LEN) sel = 1u, wt = sd_words(ql) + sd_words(tl);
        },
        [&](uint64_t i, uint64_t r, uint64_t wo) {
            S.l_id[r] = (uint32_t)i, S.l_qw[r] = wo, S.l_tw[r] = wo + sd_words(S.q_len[i]), S.l_bad[r] = 0u;
        });
    if constexpr (!WRITE) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) mx = umax2(mx, (uint32_t)__shfl_xor((int)mx, d, 64));
        if ((threadIdx.x & 63u) == 0u && mx != 0u) atomicMax(&S.ctl[SDC_MAX_LEN], (unsigned long long)mx);
        if (oob) atomicOr(&S.ctl[SDC_BOUNDS], 1ull);
    }
}

// ---- packing.  pack8: eight bytes -> 16 bits of codes (byte >> 1) & 3; `bad` collects the difference between each byte and the
// canonical letter of its code (pack8 / pack_seq_fast of wfa_entry.hip, same arithmetic)
__device__ inline uint32_t sd_pack8(uint64_t w, uint64_t &bad) {
    const uint64_t x = (w >> 1) & 0x0303030303030303ull;
    const uint64_t t = (x >> 1) & ~x & 0x0101010101010101ull;  // code 2 = 'T'
    bad |= (0x4141414141414141ull + 2 * x + 15 * t) ^ w;
    uint64_t y = (x | (x >> 6)) & 0x000F000F000F000Full;
    y          = (y | (y >> 12)) & 0x000000FF000000FFull;
    return (uint32_t)((y | (y >> 24)) & 0xFFFFull);
}
// the 16 bytes at the 16-byte aligned address a; what lies outside [lo, hi) -- only ever the first or the last granule of the
// caller's buffer -- is not read and comes back as zero
__device__ inline uint4 sd_load16(const uint8_t *a, const uint8_t *lo, const uint8_t *hi) {
    if (WFA_OFTEN(a >= lo && a + 16 <= hi)) return *reinterpret_cast<const uint4 *>(a);
    uint32_t v[4] = {0u, 0u, 0u, 0u};
    for (int b = 0; b < 16; b++)
        if (a + b >= lo && a + b < hi) v[b >> 2] |= (uint32_t)a[b] << (8 * (b & 3));
    return make_uint4(v[0], v[1], v[2], v[3]);
}

// S.n = long pairs; sequence s of the launch is the query (s even) or the target (s odd) of long pair s / 2
__global__ __launch_bounds__(SD_BLOCK) void wfa_score_pack_kernel(const SDParams S) {
    const uint8_t *const lo = S.blob, *const hi = S.blob + S.blob_bytes;
    for (uint64_t s = blockIdx.x; s < 2ull * S.n; s += gridDim.x) {
        const uint64_t  j   = s >> 1;
        const uint32_t  i   = S.l_id[j];
        const bool      tgt = (s & 1ull) != 0ull;
        const uint32_t  len = tgt ? S.t_len[i] : S.q_len[i];
        const uint8_t  *src = S.blob + (tgt ? S.t_off[i] : S.q_off[i]);
        uint32_t *const dst = S.words + (tgt ? S.l_tw[j] : S.l_qw[j]);
        const uint32_t  sh  = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15u);  // the sequence starts sh bytes into a granule
        const uint8_t *const a0 = src - sh;
        const uint32_t  nw = (len + 15u) >> 4, ds = sh >> 2, bs = (sh & 3u) * 8u;
        uint64_t        bad = 0ull;
        for (uint32_t w = threadIdx.x; w < nw; w += SD_BLOCK) {
            const uint32_t nb = umin2(16u, len - 16u * w);  // bytes of the sequence in this word
            const uint4    A  = sd_load16(a0 + 16ull * w, lo, hi);
            uint4          B  = make_uint4(0u, 0u, 0u, 0u);
            if (sh + nb > 16u) B = sd_load16(a0 + 16ull * w + 16u, lo, hi);
            const uint32_t v[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
            uint32_t       u[5], o[4];
#pragma unroll
            for (int k = 0; k < 5; k++) u[k] = ds == 0u ? v[k] : (ds == 1u ? v[k + 1] : (ds == 2u ? v[k + 2] : v[k + 3]));
#pragma unroll
            for (int k = 0; k < 4; k++) o[k] = __funnelshift_r(u[k], u[k + 1], bs);
            uint64_t x0 = (uint64_t)o[0] | ((uint64_t)o[1] << 32), x1 = (uint64_t)o[2] | ((uint64_t)o[3] << 32);
            if (nb < 16u) {  // the last word: 'A' (code 0) beyond the sequence, as pack_seq_fast's tail
                const uint32_t n0 = umin2(nb, 8u), n1 = nb - n0;
                const uint64_t m0 = n0 == 8u ? ~0ull : (1ull << (8u * n0)) - 1ull, m1 = n1 == 8u ? ~0ull : (1ull << (8u * n1)) - 1ull;
                x0 = (x0 & m0) | (0x4141414141414141ull & ~m0), x1 = (x1 & m1) | (0x4141414141414141ull & ~m1);
            }
            dst[w] = sd_pack8(x0, bad) | (sd_pack8(x1, bad) << 16);
        }
        if (threadIdx.x == 0) dst[nw] = 0u;  // the pad word
        if (bad != 0ull) atomicOr(&S.l_bad[j], 1u);
    }
}

// S.n = long pairs
template <bool WRITE>
__global__ __launch_bounds__(SD_BLOCK) void wfa_score_list_kernel(const SDParams S) {
    sd_select<WRITE>(
        S,
        [&](uint64_t j, uint32_t &sel, uint64_t &wt) {
            sel = S.l_bad[j] == 0u ? 1u : 0u, wt = 0ull;
            if constexpr (WRITE)
                if (!sel) S.score_out[S.l_id[j]] = make_uint2(ST_REDO_BYTES, 0u);
        },
        [&](uint64_t j, uint64_t r, uint64_t) {
            const uint32_t i = S.l_id[j];
            const uint64_t qw = S.l_qw[j], tw = S.l_tw[j];
            S.table[2ull * r]        = make_uint4((uint32_t)qw, (uint32_t)(qw >> 32), S.q_len[i], i);
            S.table[2ull * r + 1ull] = make_uint4((uint32_t)tw, (uint32_t)(tw >> 32), S.t_len[i], 0u);
        });
}

template <bool WRITE>
__global__ __launch_bounds__(SD_BLOCK) void wfa_score_redo_kernel(const SDParams S) {
    uint32_t mx = 0u;
    sd_select<WRITE>(
        S,
        [&](uint64_t i, uint32_t &sel, uint64_t &wt) {
            sel = (S.all != 0u || S.score_out[i].x >= (uint32_t)ST_REDO_BYTES) ? 1u : 0u;
            if (!sel) return;
            const uint32_t ql = S.q_len[i], tl = S.t_len[i];
            if (sd_valid(ql, tl)) wt = (uint64_t)ql + tl, mx = umax2(mx, umax2(ql, tl));
        },
        [&](uint64_t i, uint64_t r, uint64_t) {
            S.r_id[r] = (uint32_t)i, S.r_qoff[r] = S.q_off[i], S.r_toff[r] = S.t_off[i], S.r_qlen[r] = S.q_len[i], S.r_tlen[r] = S.t_len[i];
        });
    if constexpr (!WRITE) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) mx = umax2(mx, (uint32_t)__shfl_xor((int)mx, d, 64));
        if ((threadIdx.x & 63u) == 0u && mx != 0u) atomicMax(&S.ctl[SDC_REDO_MAX], (unsigned long long)mx);
    }
}

// S.rec == nullptr: pair i of S.n from score_out[i] (the pairs of the full path are left for the launches below);
// else: pair r_id[first + j] from record j of S.n records of the full path
__global__ __launch_bounds__(SD_BLOCK) void wfa_score_finish_kernel(const SDParams S) {
    const uint64_t j = (uint64_t)blockIdx.x * SD_BLOCK + threadIdx.x;
    if (j >= S.n) return;
    if (S.rec == nullptr) {
        const uint2 r = S.score_out[j];
        if (r.x >= (uint32_t)ST_REDO_BYTES) return;
        S.d_status[j] = (int32_t)r.x, S.d_score[j] = r.x == (uint32_t)ST_OK ? r.y : 0u;
        return;
    }
    const uint32_t i  = S.r_id[S.first + j];
    uint32_t       st = S.rec[j * REC_WORDS + REC_STATUS], sc = S.rec[j * REC_WORDS + REC_SCORE];
    // (unpack_results' rule; the full path ran under the call's bound and has said ST_OVER_MAX itself)
    if (!(st == (uint32_t)ST_OK || st == (uint32_t)ST_EMPTY || st == (uint32_t)ST_TOO_LONG || st == (uint32_t)ST_OVER_MAX)) st = ST_NO_MEMORY;
    S.d_status[i] = (int32_t)st, S.d_score[i] = st == (uint32_t)ST_OK ? sc : 0u;
}

// ---- wfahip_score_batch_packed_device: the same routing for a batch of caller-packed words in HBM with a reverse-complement flag per
// pair (wfa_score_entry.hip: score_batch_packed_device_impl).  Packed input has no byte outside ACGT, so there is neither a pack nor a
// list stage: the plan's write launch emits wfa_score_long_kernel's table directly, its offsets pointing INTO the caller's words.
//   wfa_score_pkplan_kernel  the bounds check in WORDS (wfa_packed_check_kernel's comparison: no sum that can wrap), the longest read,
//                            whether a flag is set, and the long pairs of a global call -- each weighs wfahip_packed_words(q_len) when it
//                            is flagged, else nothing: the scan then places the reverse complements in S.rc_words
//   wfa_score_rcq_kernel     writes them: a workgroup per listed pair (an unflagged one leaves at once), a lane per word through rc_word,
//                            a zero pad word.  One reverse complement per flagged long pair: no dedup by {offset, length}
//   wfa_score_pkredo_kernel  the pairs handed back, weighing the words wfahip_pack_pairs would give them (an empty or too long pair: one
//                            zero word per sequence); its write launch emits fresh word offsets, the lengths and the flag
//   wfa_score_gather_kernel  copies exactly those pairs' words to the fresh offsets, a wave per sequence: a flagged query through rc_word,
//                            the bits beyond the last base and the pad word CLEARED (KERNELS.md 4l)
template <bool WRITE>
__global__ __launch_bounds__(SD_BLOCK) void wfa_score_pkplan_kernel(const SDParams S) {
    uint32_t mx = 0u, oob = 0u, any = 0u;
    sd_select<WRITE>(
        S,
        [&](uint64_t i, uint32_t &sel, uint64_t &wt) {
            const uint32_t ql = S.q_len[i], tl = S.t_len[i];
            const bool     fl = S.q_rc != nullptr && S.q_rc[i] != 0;
            if constexpr (!WRITE) any |= fl ? 1u : 0u;
            if (!sd_valid(ql, tl)) return;  // (empty or too long: its offsets are never looked at, whatever its flag)
            if constexpr (!WRITE) {
                const uint64_t qo = S.q_off[i], to = S.t_off[i], nw = S.n_words;
                if (qo > nw || sd_words(ql) > nw - qo || to > nw || sd_words(tl) > nw - to) oob = 1u;
                mx = umax2(mx, umax2(ql, tl));
            }
            if (S.want_long != 0u && umax2(ql, tl) > SCORE_MAX_LEN) sel = 1u, wt = fl ? sd_words(ql) : 0ull;
        },
        [&](uint64_t i, uint64_t r, uint64_t wo) {
            const bool     fl = S.q_rc != nullptr && S.q_rc[i] != 0;
            const uint64_t qw = fl ? wo : S.q_off[i], tw = S.t_off[i];
            S.table[2ull * r]        = make_uint4((uint32_t)qw, (uint32_t)(qw >> 32), S.q_len[i], (uint32_t)i);
            S.table[2ull * r + 1ull] = make_uint4((uint32_t)tw, (uint32_t)(tw >> 32), S.t_len[i], fl ? 1u : 0u);
        });
    if constexpr (!WRITE) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) mx = umax2(mx, (uint32_t)__shfl_xor((int)mx, d, 64));
        if ((threadIdx.x & 63u) == 0u && mx != 0u) atomicMax(&S.ctl[SDC_MAX_LEN], (unsigned long long)mx);
        if (oob) atomicOr(&S.ctl[SDC_BOUNDS], 1ull);
        if (any) atomicOr(&S.ctl[SDC_ANY_RC], 1ull);
    }
}

// S.n = listed long pairs; workgroup j takes pair j of S.table.  A wave writes 64 consecutive words
__global__ __launch_bounds__(SD_BLOCK) void wfa_score_rcq_kernel(const SDParams S) {
    const uint64_t j = blockIdx.x;
    if (j >= S.n) return;
    const uint4 q = S.table[2ull * j], t = S.table[2ull * j + 1ull];
    if (t.w == 0u) return;
    const uint32_t *const src = S.pk_words + S.q_off[q.w];
    uint32_t *const       dst = S.rc_words + ((uint64_t)q.y << 32 | q.x);
    const uint32_t        nw  = (q.z + 15u) >> 4;
    for (uint32_t w = threadIdx.x; w < nw; w += SD_BLOCK) dst[w] = rc_word(src, q.z, w);
    if (threadIdx.x == 0) dst[nw] = 0u;
}

template <bool WRITE>
__global__ __launch_bounds__(SD_BLOCK) void wfa_score_pkredo_kernel(const SDParams S) {
    uint32_t mx = 0u;
    sd_select<WRITE>(
        S,
        [&](uint64_t i, uint32_t &sel, uint64_t &wt) {
            sel = (S.all != 0u || S.score_out[i].x >= (uint32_t)ST_REDO_BYTES) ? 1u : 0u;
            if (!sel) return;
            const uint32_t ql = S.q_len[i], tl = S.t_len[i];
            wt = 2ull;
            if (sd_valid(ql, tl)) wt = sd_words(ql) + sd_words(tl), mx = umax2(mx, umax2(ql, tl));
        },
        [&](uint64_t i, uint64_t r, uint64_t wo) {
            const uint32_t ql = S.q_len[i], tl = S.t_len[i];
            S.r_id[r] = (uint32_t)i, S.r_qoff[r] = wo, S.r_toff[r] = wo + (sd_valid(ql, tl) ? sd_words(ql) : 1ull), S.r_qlen[r] = ql, S.r_tlen[r] = tl;
            S.r_rc[r] = (S.q_rc != nullptr && S.q_rc[i] != 0) ? 1 : 0;
        });
    if constexpr (!WRITE) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) mx = umax2(mx, (uint32_t)__shfl_xor((int)mx, d, 64));
        if ((threadIdx.x & 63u) == 0u && mx != 0u) atomicMax(&S.ctl[SDC_REDO_MAX], (unsigned long long)mx);
    }
}

// S.n = pairs of the full path; sequence s of the launch is the query (s even) or the target (s odd) of pair s / 2.  A wave per sequence
// (a batch on a shape without an instance may be 1e6 sequences of a few words), the waves of the grid striding over them; a wave
// writes 64 consecutive words a round
__global__ __launch_bounds__(SD_BLOCK) void wfa_score_gather_kernel(const SDParams S) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * (SD_BLOCK / 64) + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * (SD_BLOCK / 64);
    for (uint64_t s = wave; s < 2ull * S.n; s += n_waves) {
        const uint64_t  j   = s >> 1;
        const bool      tgt = (s & 1ull) != 0ull;
        const uint32_t  ql = S.r_qlen[j], tl = S.r_tlen[j];
        uint32_t *const dst = S.g_words + (tgt ? S.r_toff[j] : S.r_qoff[j]);
        if (!sd_valid(ql, tl)) {  // (one zero word, and the offsets of the pair are never looked at)
            if (lane == 0u) dst[0] = 0u;
            continue;
        }
        const uint32_t        i   = S.r_id[j];
        const uint32_t        len = tgt ? tl : ql, nw = (len + 15u) >> 4, tail = len & 15u;
        const uint32_t *const src = S.pk_words + (tgt ? S.t_off[i] : S.q_off[i]);
        const bool            rc  = !tgt && S.r_rc[j] != 0;
        for (uint32_t w = lane; w < nw; w += 64u) {
            uint32_t v = rc ? rc_word(src, len, w) : src[w];
            if (w == nw - 1u && tail != 0u) v &= (1u << (2u * tail)) - 1u;
            dst[w] = v;
        }
        if (lane == 0u) dst[nw] = 0u;
    }
}

// ---- wfahip_select_pairs_device: the pairs with status WFAHIP_PAIR_OK, in pair order, as the next stage's arrays
template <bool WRITE>
__global__ __launch_bounds__(SD_BLOCK) void wfa_score_select_kernel(const SDParams S) {
    sd_select<WRITE>(
        S, [&](uint64_t i, uint32_t &sel, uint64_t &wt) { sel = S.sel_status[i] == (int32_t)ST_OK ? 1u : 0u, wt = 0ull; },
        [&](uint64_t i, uint64_t r, uint64_t) {
            if (S.r_id != nullptr) S.r_id[r] = (uint32_t)i;
            S.r_qoff[r] = S.q_off[i], S.r_toff[r] = S.t_off[i], S.r_qlen[r] = S.q_len[i], S.r_tlen[r] = S.t_len[i];
            if (S.r_rc != nullptr) S.r_rc[r] = S.q_rc[i];
        });
}
#endif  // WFA_SCORE_UNIT

}  // namespace wfa
