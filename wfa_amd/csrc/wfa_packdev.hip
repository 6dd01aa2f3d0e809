// wfa_packdev.hip -- wfahip_pack_pairs_device: the 2-bit packer as kernels, for sequence bytes that already live on the device.  Its
// output is word for word what the host packer wfahip_pack_pairs writes (wfa_entry.hip: pack_pairs_impl), so that the words go
// straight into wfahip_align_batch_packed_device.  The packing rule is wfa_packdev.hpp's.
//
// Three passes:
//   1  wfa_packdev_len_kernel, a lane per pair: words(q) + words(t) into d_q_woff, and the bounds check of both sequences against
//      [0, blob_bytes) from the offset and length arrays alone;
//   2  an exclusive 64-bit scan in pair order, in place in d_q_woff (the shape of wfa_cigar.hip's scan: blocks, block sums, add); the
//      pass that adds the block bases also writes t_woff[i] = q_woff[i] + words(q_i);
//   3  wfa_packdev_pack_kernel, laid out over OUTPUT WORDS: a workgroup takes a tile of PKD_TILE words, finds the pair its first word
//      belongs to by a 64-ary search of a wave in d_q_woff, keeps the starts of the pairs that begin inside the tile in LDS (there
//      are at most PKD_TILE / 2 of them: a pair takes two words at least), and every lane makes one word at a time from 16 bytes.
//      500 reads of 50 kbp and 1e6 reads of 100 bases both fill the GPU, and every word -- pad and zero words included -- is
//      written exactly once, by the lane that owns it.
// Between passes 2 and 3 the host fetches the counters (the total and the bounds verdict): no sequence byte is read before the
// offsets are known to be inside the blob; behind pass 3 it fetches them again for the ACGT verdict.
#include "wfa_ctx.hpp"
#include "wfa_packdev.hpp"

using namespace wfa;

namespace {

constexpr int      PKD_SCAN_BLOCK = 1024, PKD_SCAN_ITEMS = 4;  // scan: pairs per block = PKD_SCAN_BLOCK * PKD_SCAN_ITEMS
constexpr uint64_t PKD_PER_BLOCK  = (uint64_t)PKD_SCAN_BLOCK * PKD_SCAN_ITEMS;
constexpr uint32_t PKD_TILE       = 1024;              // output words per workgroup of the pack pass: four per lane
constexpr uint32_t PKD_STARTS     = PKD_TILE / 2 + 2;  // pair starts a tile can see: the pair its first word lies in, the <= TILE / 2 behind it, one beyond
constexpr int      PKD_CTL_WORDS  = 8;                 // u64 counters, one 64-byte fetch
enum { PKD_TOTAL = 0, PKD_BAD_RANGE = 1, PKD_BAD_BYTE = 2 };
static_assert(PKD_CTL_WORDS * 8 <= HPIN_REDO * 4, "the counters fit the head of the pinned block");

struct PkdParams {
    const uint8_t  *blob;
    uint64_t        blob_bytes;
    const uint64_t *q_off, *t_off;  // [n]
    const uint32_t *q_len, *t_len;  // [n]
    uint64_t        n;
    uint64_t       *q_woff, *t_woff;  // [n]: q_woff holds words per pair after pass 1, the exclusive offsets after the scan
    uint32_t       *packed;
    uint64_t        total;            // pass 3: the words to write
    uint64_t       *blk_sum;          // [n_blocks]
    unsigned long long *ctl;          // [PKD_CTL_WORDS]
};

// words of a sequence as the host packer counts them: a length over WFAHIP_MAX_SEQ_LEN counts as 0
__device__ __forceinline__ uint32_t pkd_len(uint32_t len) { return len <= WFAHIP_MAX_SEQ_LEN ? len : 0u; }
__device__ __forceinline__ uint64_t pkd_words(uint32_t len) { return ((uint64_t)pkd_len(len) + 15u) / 16u + 1u; }

}  // namespace

// pass 1: words per pair, and every sequence that will be read inside [0, blob_bytes) (compared without a sum that could wrap)
__global__ __launch_bounds__(256) void wfa_packdev_len_kernel(const PkdParams K) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= K.n) return;
    const uint32_t ql = pkd_len(K.q_len[i]), tl = pkd_len(K.t_len[i]);
    K.q_woff[i] = pkd_words(ql) + pkd_words(tl);
    bool bad = false;
    if (ql != 0u) {
        const uint64_t o = K.q_off[i];
        bad = o > K.blob_bytes || ql > K.blob_bytes - o;
    }
    if (tl != 0u) {
        const uint64_t o = K.t_off[i];
        bad = bad || o > K.blob_bytes || tl > K.blob_bytes - o;
    }
    if (bad) atomicOr(&K.ctl[PKD_BAD_RANGE], 1ull);
}

// pass 2a: exclusive offsets inside a block of PKD_PER_BLOCK pairs, in place, + the block's total
__global__ __launch_bounds__(PKD_SCAN_BLOCK) void wfa_packdev_scan_blocks(const PkdParams K) {
    __shared__ unsigned long long wsum[PKD_SCAN_BLOCK / 64];
    const int      tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t i0  = ((uint64_t)blockIdx.x * PKD_SCAN_BLOCK + tid) * PKD_SCAN_ITEMS;
    unsigned long long v[PKD_SCAN_ITEMS], mine = 0ull;
#pragma unroll
    for (int k = 0; k < PKD_SCAN_ITEMS; k++) v[k] = i0 + k < K.n ? K.q_woff[i0 + k] : 0ull, mine += v[k];
    unsigned long long incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    unsigned long long wbase = 0ull;
    for (int w = 0; w < wv; w++) wbase += wsum[w];
    unsigned long long run = wbase + incl - mine;
#pragma unroll
    for (int k = 0; k < PKD_SCAN_ITEMS; k++) {
        if (i0 + k < K.n) K.q_woff[i0 + k] = run;
        run += v[k];
    }
    if (tid == PKD_SCAN_BLOCK - 1) K.blk_sum[blockIdx.x] = run;
}

// pass 2b: exclusive scan of the block sums (one block); the total lands in the counters
__global__ __launch_bounds__(1024) void wfa_packdev_scan_sums(const PkdParams K, uint32_t n_blocks) {
    __shared__ unsigned long long wsum[16];
    __shared__ unsigned long long carry;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) carry = 0ull;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += 1024) {
        const uint32_t     b    = b0 + tid;
        unsigned long long mine = b < n_blocks ? K.blk_sum[b] : 0ull, incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        unsigned long long wbase = carry;
        for (int w = 0; w < wv; w++) wbase += wsum[w];
        if (b < n_blocks) K.blk_sum[b] = wbase + incl - mine;
        __syncthreads();
        if (tid == 1023) carry = wbase + incl;
        __syncthreads();
    }
    if (tid == 0) K.ctl[PKD_TOTAL] = carry;
}

// pass 2c: the block bases added, and the targets' offsets behind their queries
__global__ __launch_bounds__(256) void wfa_packdev_scan_add(const PkdParams K) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= K.n) return;
    const uint64_t q = K.q_woff[i] + K.blk_sum[i / PKD_PER_BLOCK];
    K.q_woff[i] = q;
    K.t_woff[i] = q + pkd_words(K.q_len[i]);
}

// pass 3: the words.  Tile t is the words [t PKD_TILE, (t + 1) PKD_TILE) below K.total.
__global__ __launch_bounds__(256) void wfa_packdev_pack_kernel(const PkdParams K) {
    __shared__ uint32_t start[PKD_STARTS];  // start[k]: the first word of pair first + k, relative to the tile (0 for k = 0, PKD_TILE = at or beyond its end)
    __shared__ uint64_t s_first;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint64_t w0  = (uint64_t)blockIdx.x * PKD_TILE;
    if (tid < 64u) {
        // the last pair whose query starts at or before w0, by a 64-ary search: q_woff[lo] <= w0 < q_woff[hi] (hi = n: none beyond)
        uint64_t lo = 0, hi = K.n;
        while (hi - lo > 1) {
            const uint64_t step = (hi - lo + 63u) / 64u, idx = lo + lane * step;
            const uint64_t m    = __ballot(idx < hi && K.q_woff[idx] <= w0);  // (lane 0 probes lo itself: always set)
            const uint64_t k    = 63u - (uint32_t)__builtin_clzll(m);
            lo                  = lo + k * step;
            hi                  = hi < lo + step ? hi : lo + step;
        }
        if (tid == 0u) s_first = lo;
    }
    __syncthreads();
    const uint64_t first = s_first;
    uint32_t       cnt   = 0;  // entries of start[] that are filled; the last of them is at or beyond the tile's end, unless the pairs end before
    for (uint32_t base = 0; base < PKD_STARTS; base += 256u) {
        const uint32_t k = base + tid;
        if (k < PKD_STARTS) {
            const uint64_t i = first + k;
            uint32_t       r = PKD_TILE;
            if (k == 0u) r = 0u;
            else if (i < K.n) {
                const uint64_t d = K.q_woff[i] - w0;  // (> 0: pair `first` is the last one at or before w0)
                r                = d < PKD_TILE ? (uint32_t)d : PKD_TILE;
            }
            start[k] = r;
        }
        __syncthreads();
        cnt = base + 256u < PKD_STARTS ? base + 256u : PKD_STARTS;
        if (start[cnt - 1u] >= PKD_TILE) break;  // (uniform: read behind the barrier)
    }
    uint32_t bad = 0u;
    for (uint32_t lw = tid; lw < PKD_TILE; lw += 256u) {
        const uint64_t w = w0 + lw;
        if (w >= K.total) break;
        uint32_t a = 0u, b = cnt;  // the last k with start[k] <= lw
        while (b - a > 1u) {
            const uint32_t mid = (a + b) >> 1;
            if (start[mid] <= lw) a = mid;
            else b = mid;
        }
        const uint64_t i    = first + a;
        const uint64_t tw   = K.t_woff[i];
        const bool     is_t = w >= tw;
        const uint32_t len  = pkd_len(is_t ? K.t_len[i] : K.q_len[i]);
        const uint64_t j    = w - (is_t ? tw : K.q_woff[i]);  // word of the sequence
        uint32_t       word = 0u;                             // (the pad word, and the one word of an empty or too long sequence)
        if (j * 16u < len) {
            const uint32_t  n_in = len - (uint32_t)j * 16u < 16u ? len - (uint32_t)j * 16u : 16u;
            const uint8_t  *src  = K.blob + (is_t ? K.t_off[i] : K.q_off[i]) + j * 16u;
            const uintptr_t ad   = reinterpret_cast<uintptr_t>(src);
            uint32_t        d[4];
            if ((ad & 15u) == 0u) {  // (the whole piece: readable up to the next 16-byte boundary behind the sequence's last base)
                const uint4 v = *reinterpret_cast<const uint4 *>(src);
                d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
            } else {  // the aligned dwords that hold a byte of the piece, funnelled into place
                const uint32_t *p  = reinterpret_cast<const uint32_t *>(ad & ~uintptr_t(3));
                const uint32_t  sh = 8u * (uint32_t)(ad & 3u), nd = (n_in + (uint32_t)(ad & 3u) + 3u) / 4u;  // 1 .. 5
                uint32_t        e[5];
#pragma unroll
                for (uint32_t k = 0; k < 5u; k++) e[k] = k < nd ? p[k] : 0u;
#pragma unroll
                for (uint32_t k = 0; k < 4u; k++) d[k] = sh == 0u ? e[k] : (e[k] >> sh) | (e[k + 1] << (32u - sh));
            }
            word = pkd_word16(d, n_in, &bad);
        }
        K.packed[w] = word;
    }
    if (bad != 0u) atomicOr(&K.ctl[PKD_BAD_BYTE], 1ull);
}

namespace {

int pack_device_impl(wfahip_ctx *ctx, const void *d_seq_blob, uint64_t blob_bytes, const void *d_q_off, const void *d_q_len,
                     const void *d_t_off, const void *d_t_len, uint64_t n, void *d_packed, uint64_t words_cap, void *d_q_woff,
                     void *d_t_woff, uint64_t *n_words, hipStream_t st) {
    // (nothing in these checks dereferences the context)
    if (!ctx || (n && (!d_q_off || !d_q_len || !d_t_off || !d_t_len || !d_q_woff || !d_t_woff))) return WFAHIP_ERR_BAD_ARG;
    if ((!d_seq_blob && blob_bytes) || (!d_packed && words_cap)) return WFAHIP_ERR_BAD_ARG;
    if (n > 0xFFFFFFF0ull) return WFAHIP_ERR_BAD_ARG;  // (align_device's limit: no entry aligns more pairs)
    if (n_words) *n_words = 0;
    if (n == 0) return WFAHIP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (!st) st = ctx->stream;
    const uint32_t n_blocks = (uint32_t)((n + PKD_PER_BLOCK - 1) / PKD_PER_BLOCK);
    // layout of ctx->pkd (bytes): counters | blk_sum[n_blocks]
    int rc = ensure(ctx, ctx->pkd, PKD_CTL_WORDS * 8 + 8ull * n_blocks);
    if (rc) return rc;
    char *const sb = static_cast<char *>(ctx->pkd.p);
    PkdParams   K{};
    K.blob = static_cast<const uint8_t *>(d_seq_blob), K.blob_bytes = blob_bytes;
    K.q_off = static_cast<const uint64_t *>(d_q_off), K.t_off = static_cast<const uint64_t *>(d_t_off);
    K.q_len = static_cast<const uint32_t *>(d_q_len), K.t_len = static_cast<const uint32_t *>(d_t_len);
    K.n = n, K.q_woff = static_cast<uint64_t *>(d_q_woff), K.t_woff = static_cast<uint64_t *>(d_t_woff);
    K.packed = static_cast<uint32_t *>(d_packed);
    K.ctl = reinterpret_cast<unsigned long long *>(sb), K.blk_sum = reinterpret_cast<uint64_t *>(sb + PKD_CTL_WORDS * 8);
    // WFAHIP_DEBUG_TIMING=1 (diagnostics, as in the CIGAR entry): the passes' hipEvent times on stderr
    struct Stamps {
        hipEvent_t ev[5] = {};
        bool       on    = false;
        ~Stamps() {
            for (hipEvent_t e : ev)
                if (e) (void)hipEventDestroy(e);
        }
        void mark(int k, hipStream_t s) {
            if (on && (ev[k] || hipEventCreate(&ev[k]) == hipSuccess)) (void)hipEventRecord(ev[k], s);
        }
        float ms(int a, int b) {
            float v = 0;
            return ev[a] && ev[b] && hipEventElapsedTime(&v, ev[a], ev[b]) == hipSuccess ? v : -1.f;
        }
    } stamps;
    stamps.on = std::getenv("WFAHIP_DEBUG_TIMING") != nullptr;
    const uint32_t pair_grid = (uint32_t)((n + 255) / 256);
    HIP_TRY(hipMemsetAsync(K.ctl, 0, PKD_CTL_WORDS * 8, st));
    stamps.mark(0, st);
    hipLaunchKernelGGL(wfa_packdev_len_kernel, dim3(pair_grid), dim3(256), 0, st, K);
    stamps.mark(1, st);
    hipLaunchKernelGGL(wfa_packdev_scan_blocks, dim3(n_blocks), dim3(PKD_SCAN_BLOCK), 0, st, K);
    hipLaunchKernelGGL(wfa_packdev_scan_sums, dim3(1), dim3(1024), 0, st, K, n_blocks);
    hipLaunchKernelGGL(wfa_packdev_scan_add, dim3(pair_grid), dim3(256), 0, st, K);
    HIP_TRY(hipGetLastError());
    stamps.mark(2, st);
    // (through the context's pinned block: a pageable copy of 64 bytes costs 0.3 ms)
    uint64_t hc[PKD_CTL_WORDS];
    HIP_TRY(hipMemcpyAsync(ctx->hpin + HPIN_CTRL, K.ctl, PKD_CTL_WORDS * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::memcpy(hc, ctx->hpin + HPIN_CTRL, sizeof hc);
    if (hc[PKD_BAD_RANGE] != 0) return WFAHIP_ERR_BAD_ARG;  // (no sequence byte has been read)
    const uint64_t total = hc[PKD_TOTAL];
    if (n_words) *n_words = total;
    if (total > words_cap) return WFAHIP_ERR_OOM;
    const uint64_t tiles = (total + PKD_TILE - 1) / PKD_TILE;
    if (tiles > 0x7FFFFFFFull) return WFAHIP_ERR_UNSUPPORTED;  // (2^41 words: beyond any device's memory)
    K.total = total;
    stamps.mark(3, st);
    hipLaunchKernelGGL(wfa_packdev_pack_kernel, dim3((uint32_t)tiles), dim3(256), 0, st, K);
    HIP_TRY(hipGetLastError());
    stamps.mark(4, st);
    HIP_TRY(hipMemcpyAsync(ctx->hpin + HPIN_CTRL, K.ctl, PKD_CTL_WORDS * 8, hipMemcpyDeviceToHost, st));  // (the ACGT verdict)
    HIP_TRY(hipStreamSynchronize(st));
    std::memcpy(hc, ctx->hpin + HPIN_CTRL, sizeof hc);
    if (stamps.on)
        std::fprintf(stderr, "[wfahip] pack pairs: %llu pairs, %llu words: len %.4f ms, scan %.4f ms, pack %.4f ms\n", (unsigned long long)n,
                     (unsigned long long)total, stamps.ms(0, 1), stamps.ms(1, 2), stamps.ms(3, 4));
    return hc[PKD_BAD_BYTE] != 0 ? WFAHIP_ERR_UNSUPPORTED : WFAHIP_OK;
}

}  // namespace

extern "C" int wfahip_pack_pairs_device(wfahip_ctx *ctx, const void *d_seq_blob, uint64_t blob_bytes, const void *d_q_off,
                                        const void *d_q_len, const void *d_t_off, const void *d_t_len, uint64_t n_pairs, void *d_packed,
                                        uint64_t words_cap, void *d_q_woff, void *d_t_woff, uint64_t *n_words, void *stream) {
    WFAHIP_GUARD(pack_device_impl(ctx, d_seq_blob, blob_bytes, d_q_off, d_q_len, d_t_off, d_t_len, n_pairs, d_packed, words_cap, d_q_woff,
                                  d_t_woff, n_words, static_cast<hipStream_t>(stream)))
}
