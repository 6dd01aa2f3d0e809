// wfa_wide_plan.hpp -- the device-side plan of a semi-global batch of mixed read lengths (align_device, wfa_host.hip): which pairs
// wfa_wide_kernel is offered, in which launch.  Everything in a launch of that kernel -- rings, LDS, waves per pair, arena slot -- is
// sized by the launch's longest read, so the batch is cut into the length classes of wfa_wide.hpp (wide_class_bound()) and every class
// gets a launch of its own; what is longer than the kernel takes goes to the long-pair ladder directly.
//
// From the device-resident q_len / t_len arrays alone, a category per pair:
//   class c                the longer read is within wide_class_bound(c) and beyond wide_class_bound(c - 1); a pair with an empty or
//                          over-long (> WP_MAX_SEQ_LEN) sequence is of class 0 -- the wide kernel's prologue writes its status
//   WIDE_N_CLASSES         both sequences non-empty and within WP_MAX_SEQ_LEN, the longer one beyond WIDE_MAX_LEN: the ladder's
// and from that
//   ids[]                  per category the ascending list of its pair indices, category after category (classes, then the ladder's)
//   ctl[WPC_COUNT + c]     pairs of category c
//   ctl[WPC_LONGEST + c]   the longest read of category c (over its pairs with two valid sequences; 0: none)
// A launch without ids[] (S.ids == nullptr) stops after the scan: the counts and the longest reads alone.
//
// Three plain launches over tiles of WP_TILE pairs: count (wfa_wide_plan_count_kernel: tile sums per category -> blk[c * tiles + tile],
// the longest reads), scan (wfa_wide_plan_scan_kernel: ONE workgroup turns the tile sums into exclusive offsets into ids[], category
// after category, and leaves the totals), scatter (wfa_wide_plan_scatter_kernel).  The order within a tile comes from ballots and
// population counts within a wave and from LDS across the waves; across tiles from the scan.  No workgroup waits for another, no
// atomic decides an order (the longest reads are an atomicMax: a value, not a place).
#pragma once
#include "wfa_wide.hpp"

namespace wfa {

constexpr uint32_t WP_BLOCK = 256, WP_ITEMS = 4, WP_TILE = WP_BLOCK * WP_ITEMS;
constexpr uint32_t WP_MAX_SEQ_LEN = 0x1FFFFFFFu;  // WFAHIP_MAX_SEQ_LEN (wfa.go:186-193), as the kernels spell it
constexpr int      WP_CATS = WIDE_N_CLASSES + 1;  // the classes, then the ladder's pairs
// the control words (uint32: a batch has fewer than 2^32 pairs): one 64-byte fetch shows the host all of them
enum { WPC_COUNT = 0, WPC_LONGEST = 8, WPC_WORDS = 16 };
static_assert(WP_CATS <= WPC_LONGEST && WPC_LONGEST + WP_CATS <= WPC_WORDS, "counts, then the longest reads, in 64 bytes");

struct WPParams {
    const uint32_t *q_len, *t_len;
    uint64_t        n;      // pairs
    uint32_t        tiles;  // (n + WP_TILE - 1) / WP_TILE
    uint32_t       *blk;    // [WP_CATS * tiles]: tile sums, then (after the scan) where the tile's pairs of the category start in ids[]
    uint32_t       *ctl;    // [WPC_WORDS], zeroed before the count
    uint32_t       *ids;    // [n]
};

#ifdef WFA_WIDE_PLAN_UNIT
// category of a pair, and (pairs with two valid sequences) its longer read
__device__ inline int wp_cat(uint32_t ql, uint32_t tl, uint32_t &len) {
    len = 0u;
    if (ql == 0u || tl == 0u || ql > WP_MAX_SEQ_LEN || tl > WP_MAX_SEQ_LEN) return 0;
    len = ql > tl ? ql : tl;
    return len > WIDE_MAX_LEN ? WIDE_N_CLASSES : wide_class_of(len);
}

// A tile is taken in WP_ITEMS rounds of WP_BLOCK consecutive pairs, a thread one pair per round: pair order = (round, wave, lane).
// wp_rounds() hands every thread the category of its pair of each round (-1: beyond the batch) and fills cnt[round][wave][category]
// with the pairs of that category in that wave of that round.
__device__ inline void wp_rounds(const WPParams &S, int (&cat)[WP_ITEMS], uint32_t (&len)[WP_ITEMS], uint32_t (*cnt)[WP_BLOCK / 64][WP_CATS]) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t r = 0; r < WP_ITEMS; r++) {
        const uint64_t i = (uint64_t)blockIdx.x * WP_TILE + r * WP_BLOCK + threadIdx.x;
        cat[r] = -1, len[r] = 0u;
        if (i < S.n) cat[r] = wp_cat(S.q_len[i], S.t_len[i], len[r]);
#pragma unroll
        for (int c = 0; c < WP_CATS; c++) {
            const uint64_t b = __ballot(cat[r] == c);
            if (lane == 0u) cnt[r][wv][c] = (uint32_t)__popcll(b);
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(WP_BLOCK) void wfa_wide_plan_count_kernel(const WPParams S) {
    __shared__ uint32_t cnt[WP_ITEMS][WP_BLOCK / 64][WP_CATS];
    int      cat[WP_ITEMS];
    uint32_t len[WP_ITEMS];
    wp_rounds(S, cat, len, cnt);
    if (threadIdx.x < (uint32_t)WP_CATS) {
        uint32_t s = 0u;
        for (uint32_t r = 0; r < WP_ITEMS; r++)
            for (uint32_t w = 0; w < WP_BLOCK / 64; w++) s += cnt[r][w][threadIdx.x];
        S.blk[(uint64_t)threadIdx.x * S.tiles + blockIdx.x] = s;
    }
    // the longest read of every category: a wave maximum, then one atomicMax per wave and category present
#pragma unroll
    for (int c = 0; c < WP_CATS; c++) {
        uint32_t mx = 0u;
#pragma unroll
        for (uint32_t r = 0; r < WP_ITEMS; r++) mx = umax2(mx, cat[r] == c ? len[r] : 0u);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) mx = umax2(mx, (uint32_t)__shfl_xor((int)mx, d, 64));
        if ((threadIdx.x & 63u) == 0u && mx != 0u) atomicMax(&S.ctl[WPC_LONGEST + c], mx);
    }
}

// One workgroup.  blk[c * tiles + tile]: pairs of category c in the tile -> the place in ids[] of the first of them: the pairs of the
// categories before c, then those of c in the tiles before this one.  The totals -> ctl[WPC_COUNT + c].
__global__ __launch_bounds__(WP_BLOCK) void wfa_wide_plan_scan_kernel(const WPParams S) {
    __shared__ uint32_t wsum[WP_BLOCK / 64];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t       base = 0u;  // (the same in every thread)
    for (int c = 0; c < WP_CATS; c++) {
        uint32_t *const row   = S.blk + (uint64_t)c * S.tiles;
        const uint32_t  first = base;
        for (uint32_t b0 = 0; b0 < S.tiles; b0 += WP_BLOCK) {
            const uint32_t j = b0 + threadIdx.x;
            const uint32_t v = j < S.tiles ? row[j] : 0u;
            uint32_t       incl = v;
#pragma unroll
            for (uint32_t d = 1; d < 64u; d <<= 1) {
                const uint32_t up = __shfl_up(incl, d, 64);
                if (lane >= d) incl += up;
            }
            if (lane == 63u) wsum[wv] = incl;
            __syncthreads();
            uint32_t before = 0u, total = 0u;
#pragma unroll
            for (uint32_t w = 0; w < WP_BLOCK / 64; w++) {
                if (w < wv) before += wsum[w];
                total += wsum[w];
            }
            if (j < S.tiles) row[j] = base + before + incl - v;
            base += total;
            __syncthreads();  // (the next round writes wsum again)
        }
        if (threadIdx.x == 0u) S.ctl[WPC_COUNT + c] = base - first;
    }
}

__global__ __launch_bounds__(WP_BLOCK) void wfa_wide_plan_scatter_kernel(const WPParams S) {
    __shared__ uint32_t cnt[WP_ITEMS][WP_BLOCK / 64][WP_CATS];
    int      cat[WP_ITEMS];
    uint32_t len[WP_ITEMS];
    wp_rounds(S, cat, len, cnt);
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t r = 0; r < WP_ITEMS; r++) {
        const uint64_t i = (uint64_t)blockIdx.x * WP_TILE + r * WP_BLOCK + threadIdx.x;
        // (every lane votes in every ballot, whether it has a pair or not)
        uint32_t rank = 0u;
#pragma unroll
        for (int c = 0; c < WP_CATS; c++) {
            const uint64_t b = __ballot(cat[r] == c);
            if (cat[r] == c) rank = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        }
        if (cat[r] >= 0) {
            uint32_t before = 0u;  // pairs of the category in the rounds and waves of the tile in front of this wave's
            for (uint32_t rr = 0; rr <= r; rr++)
                for (uint32_t w = 0; w < WP_BLOCK / 64; w++)
                    if (rr < r || w < wv) before += cnt[rr][w][cat[r]];
            const uint64_t at = (uint64_t)S.blk[(uint64_t)cat[r] * S.tiles + blockIdx.x] + before + rank;
            if (at < S.n) S.ids[at] = (uint32_t)i;  // (always: the categories' counts sum to n)
        }
    }
}
#endif  // WFA_WIDE_PLAN_UNIT

}  // namespace wfa
