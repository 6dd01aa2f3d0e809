// wfa_cigar.hip -- CIGAR text rendered where the ops are (include/wfa_hip.h: wfahip_cigar_text_device, wfahip_cigar_text,
// wfahip_align_batch_text).  The rendering rule is wfa_cigar.hpp's, shared by the kernels and the host renderer.
//
// The alignment leaves a 64-byte record per pair and the pair's ops somewhere in the shared op buffer; a file writer wants
// AlignmentResult.CIGAR() of every pair.  That is the work wfa_finalize.hpp does for the result arrays once more -- a length per
// pair, a scan in pair order, a scatter -- with bytes in place of ops, and the ops are in HBM when it is needed:
//   wfa_cigar_len_kernel    a wave per pair, four pairs per block, lanes striding over the ops: the range that renders (under
//                           only_aligned the first to the last 'M' op, from ballots) and the bytes of its text (digits by compares)
//   the scan                exclusive, 64-bit, in pair order, in place in the caller's offset array: a block scan, the scan of the
//                           block sums, the bases added (wfa_cigar_scan_blocks / _sums / _add)
//   wfa_cigar_write_kernel  a wave per pair in rounds of 64 ops: each lane renders its own op, a wave prefix sum of the op lengths
//                           places it, the round's total is carried into the next round.  The bytes go straight to global memory.
//                           (A round staged in LDS and stored as aligned dwords measured 9 % slower: KERNELS.md 4p.)
// The host learns two numbers per call -- the total and whether a record points outside the op buffer -- from one 64-byte fetch.
#include "wfa_ctx.hpp"
#include "wfa_hostpack.hpp"
#include "wfa_cigar.hpp"

using namespace wfa;

namespace {

constexpr int CIG_SCAN_BLOCK = 1024, CIG_SCAN_ITEMS = 4;  // scan: pairs per block = CIG_SCAN_BLOCK * CIG_SCAN_ITEMS
constexpr uint64_t CIG_PER_BLOCK = (uint64_t)CIG_SCAN_BLOCK * CIG_SCAN_ITEMS;
constexpr int CIG_CTL_WORDS = 8;  // u64 counters, one 64-byte fetch: [0] total bytes [1] != 0: an OK record's ops leave the op buffer
enum { CIG_TOTAL = 0, CIG_BAD_RANGE = 1 };
static_assert(CIG_CTL_WORDS * 8 <= HPIN_REDO * 4, "the counters fit the head of the pinned block");

struct CigParams {
    const uint32_t *rec;   // [n][REC_WORDS]
    const uint64_t *ops;   // the op buffer the records index
    uint64_t        ops_cap, n;
    uint32_t        only_aligned;
    uint64_t       *text_off;  // [n + 1]: lengths after the first pass, exclusive offsets (and the total) after the scan
    uint8_t        *text;
    uint64_t       *blk_sum;   // [n_blocks] bytes per scan block, then exclusive bases
    uint2          *range;     // [n] {first op that renders, number of ops that render}, relative to the pair's ops
    unsigned long long *ctl;   // [CIG_CTL_WORDS]
};

}  // namespace

// pass 1: the range of each pair's ops that renders and the bytes of its text
__global__ __launch_bounds__(256) void wfa_cigar_len_kernel(const CigParams C) {
    const uint64_t i    = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (i >= C.n) return;
    const uint32_t *r   = C.rec + i * REC_WORDS;
    uint32_t        len = r[REC_STATUS] == ST_OK ? r[REC_OPS_LEN] : 0u;  // (fin_len's rule: a failed pair's record may hold stale words)
    const uint64_t  src = (uint64_t)r[REC_OPS_OFF_LO] | ((uint64_t)r[REC_OPS_OFF_HI] << 32);
    if (r[REC_STATUS] == ST_OK && (len > C.ops_cap || src > C.ops_cap - len)) {  // (compared without a sum that could wrap)
        if (lane == 0) atomicOr(&C.ctl[CIG_BAD_RANGE], 1ull);
        len = 0u;  // none of its ops is read
    }
    const uint64_t *ops = C.ops + (len != 0u ? src : 0ull);
    uint32_t first = 0u, end = len;  // the ops [first, end) render
    if (C.only_aligned != 0u) {
        first = len, end = 0u;
        for (uint32_t b = 0; b < len; b += 64u) {
            const uint32_t k = b + lane;
            const uint64_t m = __ballot(k < len && cig_is_m(ops[k]));
            if (m != 0ull) {
                if (first == len) first = b + (uint32_t)__builtin_ctzll(m);
                end = b + 64u - (uint32_t)__builtin_clzll(m);
            }
        }
        if (end == 0u) first = 0u;  // no 'M' op: nothing renders
    }
    unsigned long long bytes = 0ull;
    for (uint32_t k = first + lane; k < end; k += 64u) bytes += cig_op_bytes(ops[k]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bytes += __shfl_xor(bytes, o, 64);
    if (lane == 0) {
        C.text_off[i] = bytes;
        C.range[i]    = make_uint2(first, end - first);
    }
}

// pass 2a: exclusive offsets inside a block of CIG_PER_BLOCK pairs, in place, + the block's total (fin_scan_blocks' shape)
__global__ __launch_bounds__(CIG_SCAN_BLOCK) void wfa_cigar_scan_blocks(const CigParams C) {
    __shared__ unsigned long long wsum[CIG_SCAN_BLOCK / 64];
    const int      tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t i0  = ((uint64_t)blockIdx.x * CIG_SCAN_BLOCK + tid) * CIG_SCAN_ITEMS;
    unsigned long long v[CIG_SCAN_ITEMS], mine = 0ull;
#pragma unroll
    for (int k = 0; k < CIG_SCAN_ITEMS; k++) v[k] = i0 + k < C.n ? C.text_off[i0 + k] : 0ull, mine += v[k];
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
    for (int k = 0; k < CIG_SCAN_ITEMS; k++) {
        if (i0 + k < C.n) C.text_off[i0 + k] = run;
        run += v[k];
    }
    if (tid == CIG_SCAN_BLOCK - 1) C.blk_sum[blockIdx.x] = run;
}

// pass 2b: exclusive scan of the block sums (one block); the total lands in the counters and behind the last offset
__global__ __launch_bounds__(1024) void wfa_cigar_scan_sums(const CigParams C, uint32_t n_blocks) {
    __shared__ unsigned long long wsum[16];
    __shared__ unsigned long long carry;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) carry = 0ull;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += 1024) {
        const uint32_t     b    = b0 + tid;
        unsigned long long mine = b < n_blocks ? C.blk_sum[b] : 0ull, incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        unsigned long long wbase = carry;
        for (int w = 0; w < wv; w++) wbase += wsum[w];
        if (b < n_blocks) C.blk_sum[b] = wbase + incl - mine;
        __syncthreads();
        if (tid == 1023) carry = wbase + incl;
        __syncthreads();
    }
    if (tid == 0) C.ctl[CIG_TOTAL] = carry, C.text_off[C.n] = carry;
}

// pass 2c: the block bases added (block 0's is 0: its launch starts at the second scan block)
__global__ __launch_bounds__(256) void wfa_cigar_scan_add(const CigParams C) {
    const uint64_t i = CIG_PER_BLOCK + (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < C.n) C.text_off[i] += C.blk_sum[i / CIG_PER_BLOCK];
}

// pass 3: the text.  Lane l of round b renders op first + b + l at the pair's offset + the bytes of the ops before it.
__global__ __launch_bounds__(256) void wfa_cigar_write_kernel(const CigParams C) {
    const uint64_t i    = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (i >= C.n) return;
    const uint2 rg = C.range[i];
    if (rg.y == 0u) return;
    const uint32_t *r   = C.rec + i * REC_WORDS;
    const uint64_t *ops = C.ops + ((uint64_t)r[REC_OPS_OFF_LO] | ((uint64_t)r[REC_OPS_OFF_HI] << 32)) + rg.x;
    uint8_t        *dst = C.text + C.text_off[i];  // (the carry between rounds moves it on)
    for (uint32_t b = 0; b < rg.y; b += 64u) {
        const uint32_t k    = b + lane;
        const bool     have = k < rg.y;
        const uint64_t op   = have ? ops[k] : 0ull;
        const uint32_t mine = have ? cig_op_bytes(op) : 0u;
        uint32_t       incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(incl, o, 64);
            if (lane >= (uint32_t)o) incl += t;
        }
        if (have) cig_render(op, dst + (incl - mine));
        dst += __shfl(incl, 63, 64);  // (at most 64 x 11 bytes a round)
    }
}

namespace {

// the three passes on stream st.  Returns WFAHIP_OK with *total set and the text written; WFAHIP_ERR_OOM (total > text_cap) with
// *total set, the offsets filled and no text byte written; WFAHIP_ERR_BAD_ARG when an OK record's ops leave the op buffer.
int cigar_device_impl(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap, uint64_t n, int only_aligned, void *d_text,
                      uint64_t text_cap, void *d_text_off, uint64_t *total, hipStream_t st) {
    const uint32_t n_blocks = (uint32_t)((n + CIG_PER_BLOCK - 1) / CIG_PER_BLOCK);
    // layout of ctx->cig (bytes): counters | blk_sum[n_blocks] | range[n]
    const uint64_t o_blk = CIG_CTL_WORDS * 8, o_rng = o_blk + 8ull * n_blocks;
    int rc = ensure(ctx, ctx->cig, o_rng + 8ull * n);
    if (rc) return rc;
    char *const sb = static_cast<char *>(ctx->cig.p);
    CigParams   C{};
    C.rec = static_cast<const uint32_t *>(d_rec), C.ops = static_cast<const uint64_t *>(d_ops), C.ops_cap = ops_cap, C.n = n;
    C.only_aligned = only_aligned ? 1u : 0u;
    C.text_off = static_cast<uint64_t *>(d_text_off), C.text = static_cast<uint8_t *>(d_text);
    C.ctl = reinterpret_cast<unsigned long long *>(sb), C.blk_sum = reinterpret_cast<uint64_t *>(sb + o_blk);
    C.range = reinterpret_cast<uint2 *>(sb + o_rng);
    const uint32_t pair_grid = (uint32_t)((n + 3) / 4);
    // WFAHIP_DEBUG_TIMING=1 (diagnostics, as in the host entry): the passes' hipEvent times on stderr
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
    HIP_TRY(hipMemsetAsync(C.ctl, 0, CIG_CTL_WORDS * 8, st));
    stamps.mark(0, st);
    hipLaunchKernelGGL(wfa_cigar_len_kernel, dim3(pair_grid), dim3(256), 0, st, C);
    stamps.mark(1, st);
    hipLaunchKernelGGL(wfa_cigar_scan_blocks, dim3(n_blocks), dim3(CIG_SCAN_BLOCK), 0, st, C);
    hipLaunchKernelGGL(wfa_cigar_scan_sums, dim3(1), dim3(1024), 0, st, C, n_blocks);
    if (n > CIG_PER_BLOCK) hipLaunchKernelGGL(wfa_cigar_scan_add, dim3((uint32_t)((n - CIG_PER_BLOCK + 255) / 256)), dim3(256), 0, st, C);
    HIP_TRY(hipGetLastError());
    stamps.mark(2, st);
    // (through the context's pinned block: a pageable copy of 64 bytes costs 0.3 ms)
    HIP_TRY(hipMemcpyAsync(ctx->hpin + HPIN_CTRL, C.ctl, CIG_CTL_WORDS * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    uint64_t hc[CIG_CTL_WORDS];
    std::memcpy(hc, ctx->hpin + HPIN_CTRL, sizeof hc);
    if (hc[CIG_BAD_RANGE] != 0) return WFAHIP_ERR_BAD_ARG;
    *total = hc[CIG_TOTAL];
    if (hc[CIG_TOTAL] > text_cap) return WFAHIP_ERR_OOM;
    if (hc[CIG_TOTAL] == 0) return WFAHIP_OK;
    stamps.mark(3, st);
    hipLaunchKernelGGL(wfa_cigar_write_kernel, dim3(pair_grid), dim3(256), 0, st, C);
    HIP_TRY(hipGetLastError());
    stamps.mark(4, st);
    HIP_TRY(hipStreamSynchronize(st));
    if (stamps.on)
        std::fprintf(stderr, "[wfahip] cigar text: %llu pairs, %llu bytes: len %.4f ms, scan %.4f ms, write %.4f ms\n", (unsigned long long)n,
                     (unsigned long long)hc[CIG_TOTAL], stamps.ms(0, 1), stamps.ms(1, 2), stamps.ms(3, 4));
    return WFAHIP_OK;
}

int cigar_text_device_entry(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap, uint64_t n_pairs, int only_aligned,
                            void *d_text, uint64_t text_cap, void *d_text_off, uint64_t *text_needed, hipStream_t st) {
    // (nothing in these checks dereferences the context)
    if (!ctx || (n_pairs && (!d_rec || !d_text_off)) || (!d_ops && ops_cap) || (!d_text && text_cap)) return WFAHIP_ERR_BAD_ARG;
    if (n_pairs > 0xFFFFFFF0ull) return WFAHIP_ERR_BAD_ARG;  // (align_device's limit: no entry leaves records of more pairs)
    if (text_needed) *text_needed = 0;
    if (n_pairs == 0 && !d_text_off) return WFAHIP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (!st) st = ctx->stream;
    if (n_pairs == 0) {
        HIP_TRY(hipMemsetAsync(d_text_off, 0, 8, st));
        HIP_TRY(hipStreamSynchronize(st));
        return WFAHIP_OK;
    }
    uint64_t  total = 0;
    const int rc    = cigar_device_impl(ctx, d_rec, d_ops, ops_cap, n_pairs, only_aligned, d_text, text_cap, d_text_off, &total, st);
    if (text_needed && (rc == WFAHIP_OK || rc == WFAHIP_ERR_OOM)) *text_needed = total;
    return rc;
}

void cigars_zero(wfahip_cigars *c) { std::memset(c, 0, sizeof *c); }

int cigar_text_host(const wfahip_results *r, int only_aligned, int n_threads, wfahip_cigars *out) {
    if (out) cigars_zero(out);
    if (!r || !out) return WFAHIP_ERR_BAD_ARG;
    const uint64_t n = r->n;
    if (n && (!r->status || !r->ops_off || !r->ops_len)) return WFAHIP_ERR_BAD_ARG;
    if (!r->ops && r->n_ops) return WFAHIP_ERR_BAD_ARG;
    if (n > (SIZE_MAX / 8) - 1) return WFAHIP_ERR_OOM;
    uint64_t *const off = static_cast<uint64_t *>(std::malloc((size_t)(n + 1) * 8));
    if (!off) return WFAHIP_ERR_OOM;
    off[n] = 0;
    // threads over contiguous ranges of pairs: the lengths (kept in off[]) and each range's sum, then -- the bases of the ranges
    // known -- the offsets and the text
    const unsigned        T   = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(1, n_threads), n));
    const uint64_t        per = T ? (n + T - 1) / T : 0;
    std::vector<uint64_t> part(T + 1, 0);
    std::atomic<int>      bad{0};
    const bool            trim = only_aligned != 0;
    const auto pair_ops = [&](uint64_t i, uint32_t *first, uint32_t *count) -> const uint64_t * {
        const uint32_t len = r->status[i] == WFAHIP_PAIR_OK ? r->ops_len[i] : 0u;
        if (len == 0u) {
            *first = *count = 0u;
            return nullptr;
        }
        const uint64_t *ops = r->ops + r->ops_off[i];
        cig_range(ops, len, trim, first, count);
        return ops + *first;
    };
    uint64_t *const part_p = part.data();
    parallel_ranges(0, T, T, [&, part_p](uint64_t t0, uint64_t t1) {
        for (uint64_t t = t0; t < t1; t++) {
            const uint64_t a = std::min(n, t * per), b = std::min(n, a + per);
            uint64_t       sum = 0;
            for (uint64_t i = a; i < b; i++) {
                if (r->status[i] == WFAHIP_PAIR_OK && (r->ops_len[i] > r->n_ops || r->ops_off[i] > r->n_ops - r->ops_len[i])) {
                    bad = 1;  // (compared without a sum that could wrap; none of this pair's ops is read)
                    off[i] = 0;
                    continue;
                }
                uint32_t        first, count;
                const uint64_t *ops = pair_ops(i, &first, &count);
                off[i] = count ? cig_text_bytes(ops, count) : 0;
                sum += off[i];
            }
            part_p[t + 1] = sum;
        }
    });
    if (bad) {
        std::free(off);
        return WFAHIP_ERR_BAD_ARG;
    }
    for (unsigned t = 0; t < T; t++) part[t + 1] += part[t];
    const uint64_t total = part[T];
    char          *text  = nullptr;
    if (total) {
        text = static_cast<char *>(std::malloc((size_t)total));
        if (!text) {
            std::free(off);
            return WFAHIP_ERR_OOM;
        }
    }
    parallel_ranges(0, T, T, [&, part_p](uint64_t t0, uint64_t t1) {
        for (uint64_t t = t0; t < t1; t++) {
            const uint64_t a = std::min(n, t * per), b = std::min(n, a + per);
            uint64_t       run = part_p[t];
            for (uint64_t i = a; i < b; i++) {
                const uint64_t bytes = off[i];
                off[i]               = run;
                if (bytes) {
                    uint32_t        first, count;
                    const uint64_t *ops = pair_ops(i, &first, &count);
                    cig_text_write(ops, count, reinterpret_cast<uint8_t *>(text) + run);
                }
                run += bytes;
            }
        }
    });
    off[n]       = total;
    out->n       = n;
    out->n_bytes = total;
    out->text    = text;
    out->off     = off;
    return WFAHIP_OK;
}

// wfahip_align_batch_text: the plain path of wfahip_align_batch with the text kernels in place of the result assembly
int align_batch_text_impl(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *seq_blob, uint64_t blob_bytes, const uint64_t *q_off,
                          const uint32_t *q_len, const uint64_t *t_off, const uint32_t *t_len, uint64_t n_pairs, int only_aligned,
                          wfahip_results *out, wfahip_cigars *cig) {
    if (cig) cigars_zero(cig);
    if (!ctx || !out || !cig) return WFAHIP_ERR_BAD_ARG;
    results_zero(out);
    int rc = check_params(p);
    if (rc) return rc;
    if (n_pairs == 0) {
        cig->off = static_cast<uint64_t *>(std::calloc(1, 8));
        return cig->off ? WFAHIP_OK : WFAHIP_ERR_OOM;
    }
    if (!q_off || !q_len || !t_off || !t_len || (!seq_blob && blob_bytes)) return WFAHIP_ERR_BAD_ARG;
    if (n_pairs > 0xFFFFFFF0ull) return WFAHIP_ERR_BAD_ARG;
    // (the last of the whole-call errors: nothing above or in this loop dereferences the context)
    uint32_t max_len = 1;
    uint64_t sum_len = 0;
    for (uint64_t i = 0; i < n_pairs; i++) {
        if (q_len[i] <= WFAHIP_MAX_SEQ_LEN && t_len[i] <= WFAHIP_MAX_SEQ_LEN && q_len[i] && t_len[i]) {
            if (q_off[i] > blob_bytes || q_len[i] > blob_bytes - q_off[i] || t_off[i] > blob_bytes || t_len[i] > blob_bytes - t_off[i])
                return WFAHIP_ERR_BAD_ARG;
            max_len = std::max(max_len, std::max(q_len[i], t_len[i]));
            sum_len += (uint64_t)q_len[i] + t_len[i];
        }
    }
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // ---- one upload (+32 bytes: aligned dword loads at the blob's tail stay inside the allocation)
    if ((rc = ensure(ctx, ctx->in_blob, blob_bytes + 32))) return rc;
    if ((rc = ensure(ctx, ctx->in_qoff, n_pairs * 8))) return rc;
    if ((rc = ensure(ctx, ctx->in_toff, n_pairs * 8))) return rc;
    if ((rc = ensure(ctx, ctx->in_qlen, n_pairs * 4))) return rc;
    if ((rc = ensure(ctx, ctx->in_tlen, n_pairs * 4))) return rc;
    if ((rc = ensure(ctx, ctx->out_rec, n_pairs * REC_WORDS * 4))) return rc;
    if (blob_bytes) HIP_TRY(hipMemcpyAsync(ctx->in_blob.p, seq_blob, blob_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->in_qoff.p, q_off, n_pairs * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->in_toff.p, t_off, n_pairs * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->in_qlen.p, q_len, n_pairs * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->in_tlen.p, t_len, n_pairs * 4, hipMemcpyHostToDevice, st));
    // ---- the alignment.  CIGAR ops are merged runs: a first guess of (n+m)/4 + 8 per pair, grown on demand (the host entry's rule)
    uint64_t ops_cap = sum_len / 4 + 8 * n_pairs + 1024;
    for (int attempt = 0; attempt < 6; attempt++) {
        if ((rc = ensure(ctx, ctx->out_ops, ops_cap * 8))) return rc;
        uint64_t needed = 0;
        rc = align_device(ctx, p, ctx->in_blob.p, blob_bytes, ctx->in_qoff.p, ctx->in_qlen.p, ctx->in_toff.p, ctx->in_tlen.p, n_pairs, max_len,
                          ctx->out_rec.p, ctx->out_ops.p, ops_cap, &needed, st, false);
        if (rc == WFAHIP_ERR_OOM && needed > ops_cap) {
            ops_cap = needed + needed / 3 + 1024;
            continue;
        }
        break;
    }
    if (rc) return rc;
    // ---- the text: sized by the first two passes, written by a second call once its buffer is there (the lengths are cheap to
    // make again; an op renders to at most 11 bytes, but a buffer for that bound would be three times the text of typical ops)
    if ((rc = ensure(ctx, ctx->cig_off, (n_pairs + 1) * 8))) return rc;
    uint64_t total = 0;
    rc = cigar_device_impl(ctx, ctx->out_rec.p, ctx->out_ops.p, ops_cap, n_pairs, only_aligned, ctx->cig_text.p, ctx->cig_text.bytes,
                           ctx->cig_off.p, &total, st);
    if (rc == WFAHIP_ERR_OOM && total > ctx->cig_text.bytes) {
        if ((rc = ensure(ctx, ctx->cig_text, total + total / 8))) return rc;
        rc = cigar_device_impl(ctx, ctx->out_rec.p, ctx->out_ops.p, ops_cap, n_pairs, only_aligned, ctx->cig_text.p, ctx->cig_text.bytes,
                               ctx->cig_off.p, &total, st);
    }
    if (rc) return rc == WFAHIP_ERR_BAD_ARG ? WFAHIP_ERR_INTERNAL : rc;  // (the records are the library's own)
    // ---- one download: records, offsets, text
    std::vector<uint32_t> rec((size_t)n_pairs * REC_WORDS);
    cig->off = static_cast<uint64_t *>(std::malloc((size_t)(n_pairs + 1) * 8));
    if (total) cig->text = static_cast<char *>(std::malloc((size_t)total));
    const auto fail = [&](int code) {
        wfahip_results_free(out);
        std::free(cig->text), std::free(cig->off);
        cigars_zero(cig);
        return code;
    };
    if (!cig->off || (total && !cig->text)) return fail(WFAHIP_ERR_OOM);
    hipError_t e = hipMemcpyAsync(rec.data(), ctx->out_rec.p, rec.size() * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(cig->off, ctx->cig_off.p, (size_t)(n_pairs + 1) * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && total) e = hipMemcpyAsync(cig->text, ctx->cig_text.p, (size_t)total, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        std::snprintf(ctx->last_error, sizeof ctx->last_error, "%s: download -> %s", __FILE__, hipGetErrorString(e));
        return fail(e == hipErrorOutOfMemory ? WFAHIP_ERR_OOM : WFAHIP_ERR_HIP);
    }
    cig->n = n_pairs, cig->n_bytes = total;
    // ---- the records unpacked (unpack_results' field rules: every field of a pair that is not OK is 0; here ops_off is 0 too)
    out->n = n_pairs;
#define ALLOC(field, type)                                                \
    out->field = static_cast<type *>(std::calloc(n_pairs, sizeof(type))); \
    if (!out->field) return fail(WFAHIP_ERR_OOM);
    ALLOC(status, int32_t) ALLOC(score, uint32_t) ALLOC(tbegin, int32_t) ALLOC(tend, int32_t)
    ALLOC(qbegin, int32_t) ALLOC(qend, int32_t) ALLOC(align_len, uint32_t) ALLOC(matches, uint32_t)
    ALLOC(gaps, uint32_t) ALLOC(gap_regions, uint32_t) ALLOC(ops_off, uint64_t) ALLOC(ops_len, uint32_t)
#undef ALLOC
    uint64_t cells = 0;
    for (uint64_t i = 0; i < n_pairs; i++) {
        const uint32_t *r  = &rec[i * REC_WORDS];
        const uint32_t  s  = r[REC_STATUS];
        out->status[i]     = (s == ST_OK || s == ST_EMPTY || s == ST_TOO_LONG || s == ST_OVER_MAX) ? (int32_t)s : WFAHIP_PAIR_NO_MEMORY;
        if (s != ST_OK) continue;
        out->score[i]       = r[REC_SCORE];
        out->tbegin[i]      = (int32_t)r[REC_TBEGIN];
        out->tend[i]        = (int32_t)r[REC_TEND];
        out->qbegin[i]      = (int32_t)r[REC_QBEGIN];
        out->qend[i]        = (int32_t)r[REC_QEND];
        out->align_len[i]   = r[REC_ALIGN_LEN];
        out->matches[i]     = r[REC_MATCHES];
        out->gaps[i]        = r[REC_GAPS];
        out->gap_regions[i] = r[REC_GAP_REGIONS];
        out->ops_len[i]     = r[REC_OPS_LEN];
        cells += (uint64_t)r[REC_CELLS_LO] | ((uint64_t)r[REC_CELLS_HI] << 32);
    }
    ctx->timing.cells_stored = cells;
    return WFAHIP_OK;
}

}  // namespace

extern "C" int wfahip_cigar_text_device(wfahip_ctx *ctx, const void *d_rec, const void *d_ops, uint64_t ops_cap, uint64_t n_pairs,
                                        int only_aligned, void *d_text, uint64_t text_cap, void *d_text_off, uint64_t *text_needed,
                                        void *stream) {
    WFAHIP_GUARD(cigar_text_device_entry(ctx, d_rec, d_ops, ops_cap, n_pairs, only_aligned, d_text, text_cap, d_text_off, text_needed,
                                         static_cast<hipStream_t>(stream)))
}

extern "C" int wfahip_cigar_text(const wfahip_results *r, int only_aligned, int n_threads, wfahip_cigars *out) {
    WFAHIP_GUARD(cigar_text_host(r, only_aligned, n_threads, out))
}

extern "C" void wfahip_cigars_free(wfahip_cigars *c) {
    if (!c) return;
    std::free(c->text), std::free(c->off);
    cigars_zero(c);
}

extern "C" int wfahip_align_batch_text(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *seq_blob, uint64_t blob_bytes,
                                       const uint64_t *q_off, const uint32_t *q_len, const uint64_t *t_off, const uint32_t *t_len,
                                       uint64_t n_pairs, int only_aligned, wfahip_results *out, wfahip_cigars *cig) {
    WFAHIP_GUARD(align_batch_text_impl(ctx, p, seq_blob, blob_bytes, q_off, q_len, t_off, t_len, n_pairs, only_aligned, out, cig))
}
