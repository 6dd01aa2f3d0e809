// wfa_entry.hip -- the host entries of the C-ABI (include/wfa_hip.h): wfahip_align_batch -- host blobs in, host result arrays out,
// with the upload, the alignment (align_device, wfa_host.hip) and the download of consecutive slices overlapped --, pre-packed
// input, wfahip_align_pair, submit / collect, and the cache the result arrays circulate through.
#define WFA_NO_AUX_KERNELS 1  // (device functions and constants of the kernels' headers only: the kernels are launched by wfa_host.hip)
#include "wfa_ctx.hpp"
#include "wfa_generic.hpp"
#include "wfa_packed.hpp"
#include "wfa_blk.hpp"
#include "wfa_duo_cfg.hpp"
#include "wfa_lane.hpp"
#include "wfa_fwd.hpp"
#include "wfa_long.hpp"
#include "wfa_finalize.hpp"
#include "wfa_wide.hpp"
#include "wfa_score.hpp"
#include "wfa_score_long.hpp"
#include "wfa_score_dev.hpp"

using namespace wfa;

void results_zero(wfahip_results *r) { std::memset(r, 0, sizeof *r); }

// Result arrays are malloc blocks OWNED BY THE LIBRARY: a binding must hand them back through wfahip_results_free and
// never free() them itself -- blocks that circulate through the cache below are page-locked (hipHostRegister), and
// freeing a registered block behind the runtime's back leaves a stale registration.  wfahip_results_free keeps the
// large ones for the next call instead of returning them to the system: a fresh 0.7 GB ops array costs its download
// twice over in first-touch page faults (the reference recycles its results the same way, wfa_cigar.go:92).
namespace {
struct ResBlock { void *p; size_t bytes; };
std::mutex            g_res_mu;
std::vector<ResBlock> g_res_cache;
size_t                g_res_cached_bytes = 0;
constexpr size_t      RES_CACHE_MIN = 1u << 20, RES_CACHE_MAX_BYTES = 4ull << 30, RES_CACHE_MAX_BLOCKS = 32;

// Blocks that come back from the cache are page-locked (hipHostRegister, once per block): the result download then
// goes straight into them at link rate -- through pinned staging plus copy-out threads 0.8 GB of results took 36 ms of
// a 44 ms call.  They stay registered while they circulate between wfahip_results_free and the next call.
std::vector<ResBlock> g_res_pinned;  // (guarded by g_res_mu)
bool res_is_pinned(const void *p, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_res_mu);
    for (const ResBlock &b : g_res_pinned)
        if (p >= b.p && static_cast<const char *>(p) + bytes <= static_cast<const char *>(b.p) + b.bytes) return true;
    return false;
}
void *res_alloc(size_t bytes) {
    if (bytes >= RES_CACHE_MIN) {
        std::lock_guard<std::mutex> lk(g_res_mu);
        size_t best = g_res_cache.size();
        for (size_t i = 0; i < g_res_cache.size(); i++)
            if (g_res_cache[i].bytes >= bytes && g_res_cache[i].bytes <= 2 * bytes &&
                (best == g_res_cache.size() || g_res_cache[i].bytes < g_res_cache[best].bytes))
                best = i;
        if (best != g_res_cache.size()) {
            void *p = g_res_cache[best].p;
            const size_t cap = g_res_cache[best].bytes;
            g_res_cached_bytes -= cap;
            g_res_cache.erase(g_res_cache.begin() + (long)best);
            bool pinned = false;
            for (const ResBlock &b : g_res_pinned) pinned = pinned || b.p == p;
            if (!pinned && !std::getenv("WFAHIP_NO_PINNED_RESULTS") &&
                hipHostRegister(p, cap, hipHostRegisterPortable) == hipSuccess)
                g_res_pinned.push_back({p, cap});
            else if (!pinned)
                (void)hipGetLastError();
            return p;
        }
    }
    return std::malloc(bytes);
}
void res_release(void *p) {
    if (!p) return;
    const size_t bytes = malloc_usable_size(p);  // (the block's real capacity, whatever the caller did to n / n_ops)
    if (bytes >= RES_CACHE_MIN) {
        std::lock_guard<std::mutex> lk(g_res_mu);
        if (g_res_cache.size() < RES_CACHE_MAX_BLOCKS && g_res_cached_bytes + bytes <= RES_CACHE_MAX_BYTES) {
            g_res_cache.push_back({p, bytes});
            g_res_cached_bytes += bytes;
            return;
        }
    }
    {
        std::lock_guard<std::mutex> lk(g_res_mu);
        for (size_t i = 0; i < g_res_pinned.size(); i++)
            if (g_res_pinned[i].p == p) {
                (void)hipHostUnregister(p);
                g_res_pinned.erase(g_res_pinned.begin() + (long)i);
                break;
            }
    }
    std::free(p);
}
}  // namespace

extern "C" void wfahip_results_free(wfahip_results *r) {
    if (!r) return;
    for (void *p : {(void *)r->status, (void *)r->score, (void *)r->tbegin, (void *)r->tend, (void *)r->qbegin, (void *)r->qend,
                    (void *)r->align_len, (void *)r->matches, (void *)r->gaps, (void *)r->gap_regions, (void *)r->ops_len,
                    (void *)r->ops_off, (void *)r->ops})
        res_release(p);
    results_zero(r);
}

int unpack_results(const std::vector<uint32_t> &rec, const std::vector<uint64_t> &ops, uint64_t n,
                          wfahip_results *out, uint64_t *cells_total) {
    results_zero(out);
    out->n = n;
    size_t cnt = std::max<uint64_t>(n, 1);
#define ALLOC(field, type)                                            \
    out->field = static_cast<type *>(std::calloc(cnt, sizeof(type))); \
    if (!out->field) return WFAHIP_ERR_OOM;
    ALLOC(status, int32_t) ALLOC(score, uint32_t) ALLOC(tbegin, int32_t) ALLOC(tend, int32_t)
    ALLOC(qbegin, int32_t) ALLOC(qend, int32_t) ALLOC(align_len, uint32_t) ALLOC(matches, uint32_t)
    ALLOC(gaps, uint32_t) ALLOC(gap_regions, uint32_t) ALLOC(ops_off, uint64_t) ALLOC(ops_len, uint32_t)
#undef ALLOC
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; i++)
        if (rec[i * REC_WORDS + REC_STATUS] == ST_OK) total += rec[i * REC_WORDS + REC_OPS_LEN];
    out->ops = static_cast<uint64_t *>(std::malloc(std::max<uint64_t>(total, 1) * 8));
    if (!out->ops) return WFAHIP_ERR_OOM;
    uint64_t pos = 0, cells = 0;
    for (uint64_t i = 0; i < n; i++) {  // ops are re-packed in pair order (device order is completion order)
        const uint32_t *r  = &rec[i * REC_WORDS];
        uint32_t        st = r[REC_STATUS];
        out->status[i]     = (st == ST_OK || st == ST_EMPTY || st == ST_TOO_LONG) ? (int32_t)st : WFAHIP_PAIR_NO_MEMORY;
        if (st != ST_OK) continue;
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
        out->ops_off[i]     = pos;
        uint64_t src        = (uint64_t)r[REC_OPS_OFF_LO] | ((uint64_t)r[REC_OPS_OFF_HI] << 32);
        std::memcpy(out->ops + pos, ops.data() + src, (size_t)r[REC_OPS_LEN] * 8);
        pos += r[REC_OPS_LEN];
        cells += (uint64_t)r[REC_CELLS_LO] | ((uint64_t)r[REC_CELLS_HI] << 32);
    }
    out->n_ops = pos;
    if (cells_total) *cells_total = cells;
    return WFAHIP_OK;
}

namespace {

constexpr size_t PIN_CHUNK = 32u << 20;

// Device -> pageable host memory: 32 MB pieces through two pinned buffers (full PCIe rate), copied out to their
// destination by a few host threads while the next piece is in flight (first-touch page faults of freshly
// malloc'd result arrays are what limits a plain hipMemcpy here).
int download(wfahip_ctx *ctx, void *dst, const void *src, size_t bytes, hipStream_t st) {
    if (bytes == 0) return WFAHIP_OK;
    if (res_is_pinned(dst, bytes)) {  // a recycled, page-locked result block: one copy at link rate
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return WFAHIP_OK;
    }
    for (int i = 0; i < 2; i++) {
        if (!ctx->pin[i]) HIP_TRY(hipHostMalloc(&ctx->pin[i], PIN_CHUNK, hipHostMallocDefault));
        if (!ctx->pin_ev[i]) HIP_TRY(hipEventCreateWithFlags(&ctx->pin_ev[i], hipEventDisableTiming));
    }
    // (measured on the 256-thread GPU box, 0.8 GB of results: 8 threads 72 ms, 16 threads 53 ms, 32 threads 60 ms)
    unsigned n_thr = std::max(1u, std::min(16u, std::thread::hardware_concurrency() / 2));
    if (const char *e = std::getenv("WFAHIP_DL_THREADS")) n_thr = (unsigned)std::max(1, std::atoi(e));
    const size_t   n_chk = (bytes + PIN_CHUNK - 1) / PIN_CHUNK;
    auto issue = [&](size_t c) -> hipError_t {
        const size_t off = c * PIN_CHUNK, sz = std::min(PIN_CHUNK, bytes - off);
        hipError_t   e   = hipMemcpyAsync(ctx->pin[c & 1], static_cast<const char *>(src) + off, sz, hipMemcpyDeviceToHost, st);
        return e != hipSuccess ? e : hipEventRecord(ctx->pin_ev[c & 1], st);
    };
    HIP_TRY(issue(0));
    for (size_t c = 0; c < n_chk; c++) {
        HIP_TRY(hipEventSynchronize(ctx->pin_ev[c & 1]));
        if (c + 1 < n_chk) HIP_TRY(issue(c + 1));
        const size_t off = c * PIN_CHUNK, sz = std::min(PIN_CHUNK, bytes - off);
        char        *d = static_cast<char *>(dst) + off;
        const char  *p = static_cast<const char *>(ctx->pin[c & 1]);
        if (sz < (4u << 20) || n_thr == 1) {
            std::memcpy(d, p, sz);
        } else {
            std::vector<std::thread> th;
            const size_t             part = ((sz / n_thr) + 4095) & ~size_t(4095);
            for (unsigned t = 0; t < n_thr; t++) {
                const size_t a = std::min(sz, (size_t)t * part), b = std::min(sz, a + part);
                if (b <= a) continue;
                try {
                    th.emplace_back([=] { std::memcpy(d + a, p + a, b - a); });
                } catch (...) {  // no more threads: this part is copied here
                    std::memcpy(d + a, p + a, b - a);
                }
            }
            for (auto &t : th) t.join();
        }
    }
    return WFAHIP_OK;
}

}  // namespace

// Pre-packed input (wfahip_align_batch_packed): 2-bit words -> the byte blob the kernels read, on the device.  One
// thread per word: 16 bases = one 16-byte store.  Code -> letter is the inverse of the kernels' (c >> 1) & 3.
__global__ __launch_bounds__(256) void wfa_unpack_kernel(const uint32_t *__restrict__ words, uint4 *__restrict__ bytes, uint64_t w0,
                                                         uint64_t w1) {
    const uint64_t i = w0 + (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= w1) return;
    const uint32_t w = words[i];
    uint32_t       o[4];
#pragma unroll
    for (int d = 0; d < 4; d++) {
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) v |= ((0x47544341u >> (8u * ((w >> (2 * (4 * d + b))) & 3u))) & 0xFFu) << (8 * b);  // "ACTG"[code]
        o[d] = v;
    }
    bytes[i] = make_uint4(o[0], o[1], o[2], o[3]);
}

__global__ __launch_bounds__(256) void wfa_scale_offsets_kernel(uint64_t *q_off, uint64_t *t_off, uint64_t n) {  // words -> bytes
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) q_off[i] *= 16, t_off[i] *= 16;
}

struct PackedFacts {
    uint32_t max_len;
    uint64_t sum_len;
};
// packed != nullptr: the sequences arrive 2-bit packed (word i of `packed` = bytes [16 i, 16 i + 16) of the blob the
// offsets refer to); seq_blob is not read.
static int align_batch_impl(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *seq_blob,
                            uint64_t blob_bytes, const uint64_t *q_off, const uint32_t *q_len,
                            const uint64_t *t_off, const uint32_t *t_len, uint64_t n_pairs,
                            wfahip_results *out, const uint32_t *packed = nullptr,
                            const std::function<int(uint64_t, uint64_t)> *lazy_pack = nullptr, const PackedFacts *facts = nullptr) {
    // (facts: the caller is the library itself -- it laid the packed words out pair after pair and has already validated the
    // caller's offsets and summed the lengths: the three passes over a million pairs this function would make are 3 ms of a 38 ms call)
    // (lazy_pack: `packed` is the library's own buffer and is only filled as the pipeline gets to a range of pairs --
    // lazy_pack(first, last) packs pairs [first, last) and returns 0, or 2 when it meets a byte outside ACGT)
    if (!ctx || !out) return WFAHIP_ERR_BAD_ARG;
    // (pre-packed input: q_off / t_off arrive in WORDS of 16 bases; they are uploaded as they are and scaled to byte
    // offsets on the device -- a second pair of host arrays would cost more in page faults than the alignment of a slice)
    const uint64_t osc = packed ? 16 : 1;
    results_zero(out);
    int rc = check_params(p);
    if (rc) return rc;
    if (n_pairs == 0) return WFAHIP_OK;
    if (!q_off || !q_len || !t_off || !t_len || (!seq_blob && !packed && blob_bytes)) return WFAHIP_ERR_BAD_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    // the bytes [lo, hi) of the blob -> in_blob on stream `s` (packed input: the words that hold them, then the unpack kernel)
    const auto upload_range = [&](uint64_t lo, uint64_t hi, hipStream_t s) -> hipError_t {
        if (hi <= lo) return hipSuccess;
        if (!packed) return hipMemcpyAsync(static_cast<char *>(ctx->in_blob.p) + lo, seq_blob + lo, hi - lo, hipMemcpyHostToDevice, s);
        // (the words stay words: the alignment copies them into the first pass's slots and expands only the pairs a pass reads
        // as bytes -- ctx->pk_words below; wfa_unpack_kernel, which expanded everything, is kept for option "unpack_all")
        const uint64_t w0 = lo / 16, w1 = (hi + 15) / 16;
        hipError_t     e  = hipMemcpyAsync(static_cast<uint32_t *>(ctx->in_packed.p) + w0, packed + w0, (w1 - w0) * 4, hipMemcpyHostToDevice, s);
        if (e != hipSuccess || ctx->opt_unpack_all == 0) return e;
        hipLaunchKernelGGL(wfa_unpack_kernel, dim3((uint32_t)((w1 - w0 + 255) / 256)), dim3(256), 0, s,
                           static_cast<const uint32_t *>(ctx->in_packed.p), static_cast<uint4 *>(ctx->in_blob.p), w0, w1);
        return hipGetLastError();
    };
    struct PkGuard {  // the packed words are the alignment's input for the duration of this call only
        wfahip_ctx *c;
        ~PkGuard() { c->pk_words = nullptr; }
    } pk_guard{ctx};
    // (ctx->pk_words is set once in_packed is allocated, below)

    uint32_t max_len = facts ? std::max(1u, facts->max_len) : 1;
    uint64_t sum_len = facts ? facts->sum_len : 0;
    for (uint64_t i = 0; i < n_pairs && !facts; i++) {
        if (q_len[i] <= WFAHIP_MAX_SEQ_LEN && t_len[i] <= WFAHIP_MAX_SEQ_LEN && q_len[i] && t_len[i]) {
            // (written so that a hostile 64-bit offset cannot wrap the sum around)
            if (q_off[i] > blob_bytes / osc || q_len[i] > blob_bytes - q_off[i] * osc || t_off[i] > blob_bytes / osc ||
                t_len[i] > blob_bytes - t_off[i] * osc)
                return WFAHIP_ERR_BAD_ARG;
            max_len = std::max(max_len, std::max(q_len[i], t_len[i]));
            sum_len += (uint64_t)q_len[i] + t_len[i];
        }
    }
    hipStream_t st = ctx->stream;
    // device staging (+16 bytes so aligned dword loads at the tail stay inside the allocation)
    if ((rc = ensure(ctx, ctx->in_blob, blob_bytes + 32))) return rc;
    if (packed && (rc = ensure(ctx, ctx->in_packed, (blob_bytes + 15) / 16 * 4 + 16))) return rc;
    if (packed && ctx->opt_unpack_all == 0) ctx->pk_words = static_cast<const uint32_t *>(ctx->in_packed.p);
    if ((rc = ensure(ctx, ctx->in_qoff, n_pairs * 8))) return rc;
    if ((rc = ensure(ctx, ctx->in_toff, n_pairs * 8))) return rc;
    if ((rc = ensure(ctx, ctx->in_qlen, n_pairs * 4))) return rc;
    if ((rc = ensure(ctx, ctx->in_tlen, n_pairs * 4))) return rc;
    if ((rc = ensure(ctx, ctx->out_rec, n_pairs * REC_WORDS * 4))) return rc;
    const bool dbg_t = std::getenv("WFAHIP_DEBUG_TIMING") != nullptr;
    auto       now   = [] { return std::chrono::steady_clock::now(); };
    auto       ms_of = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double, std::milli>(b - a).count();
    };
    const auto t_h2d = now();
    // Large batches: the pairs are aligned in a few slices, each as soon as the part of the blob it refers to has
    // arrived (an uploader thread feeds a copy stream), so most of the alignment time hides behind the upload.
    // Needs the blob ranges of consecutive slices to be disjoint enough (pairs laid out in order, the usual case).
    constexpr int     UP_SLICES = 6;  // (at most; packed input -- a quarter of the bytes -- is cut into three: a slice costs ~2 ms of its own)
    // (measured, 1e6 x 1 kbp packed on the fly: 4 slices 35.8 ms, 5 slices 34.8, 3 slices 39; six fall under the pair count at
    // which the variable-lanes kernel takes a pass: 46)
    int               n_sl = (packed && !lazy_pack) ? 3 : (lazy_pack && n_pairs >= 900000 ? 5 : 4);
    if (const char *e = std::getenv("WFAHIP_SLICES")) n_sl = std::max(1, std::min(UP_SLICES, std::atoi(e)));
    uint64_t          sl_first[UP_SLICES + 1], sl_lo[UP_SLICES], sl_hi[UP_SLICES];
    bool              sliced = n_pairs >= 200000 && blob_bytes >= (packed ? (256u << 20) : (64u << 20)) && !std::getenv("WFAHIP_NO_UPLOAD_OVERLAP");
    if (sliced) {
        uint64_t covered = 0;
        for (int k = 0; k <= UP_SLICES; k++) sl_first[k] = k <= n_sl ? n_pairs * k / n_sl : n_pairs;
        // (packing on the fly: nothing can be uploaded before the first slice is packed, so the first slice is a small one; and
        // the last one too: its results are downloaded with nothing left to hide them behind)
        if (lazy_pack && n_sl == 4) sl_first[1] = n_pairs * 12 / 100, sl_first[2] = n_pairs * 46 / 100, sl_first[3] = n_pairs * 80 / 100;
        if (lazy_pack && n_sl == 3) sl_first[1] = n_pairs * 14 / 100, sl_first[2] = n_pairs * 62 / 100;
        if (lazy_pack && n_sl >= 5) {  // a small first slice, a smaller last one, equal ones between
            sl_first[1] = n_pairs * 10 / 100;
            for (int k = 2; k < n_sl; k++) sl_first[k] = n_pairs * (10 + (k - 1) * 74 / (n_sl - 2)) / 100;
        }
        for (int k = 0; k < n_sl && sliced; k++) {
            uint64_t lo = blob_bytes, hi = 0;
            if (facts && sl_first[k + 1] > sl_first[k]) {  // (pair after pair: a slice's words are one range, query of its first pair .. target of its last)
                const uint64_t a = sl_first[k], b = sl_first[k + 1] - 1;
                lo = q_off[a] * osc, hi = (t_off[b] + wfahip_packed_words(t_len[b] <= WFAHIP_MAX_SEQ_LEN && q_len[b] && t_len[b] && q_len[b] <= WFAHIP_MAX_SEQ_LEN ? t_len[b] : 0)) * osc;
            }
            for (uint64_t i = sl_first[k]; i < sl_first[k + 1] && !facts; i++) {
                if (!(q_len[i] <= WFAHIP_MAX_SEQ_LEN && t_len[i] <= WFAHIP_MAX_SEQ_LEN && q_len[i] && t_len[i])) continue;
                lo = std::min(lo, std::min(q_off[i], t_off[i]) * osc);
                hi = std::max(hi, std::max(q_off[i] * osc + q_len[i], t_off[i] * osc + t_len[i]));
            }
            if (hi <= lo) lo = hi = 0;
            lo &= ~15ull;  // (whole aligned dwords of the first sequence; the tail padding of in_blob covers the end)
            sl_lo[k] = lo, sl_hi[k] = hi, covered += hi - lo;
        }
        sliced = covered <= blob_bytes + blob_bytes / 4;
    }
    if (sliced) {
        if (!ctx->stream_up) HIP_TRY(hipStreamCreateWithFlags(&ctx->stream_up, hipStreamNonBlocking));
        if (!ctx->stream_dn) HIP_TRY(hipStreamCreateWithFlags(&ctx->stream_dn, hipStreamNonBlocking));
        while (ctx->ev_up.size() < (size_t)UP_SLICES) {
            hipEvent_t e;
            HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            ctx->ev_up.push_back(e);
        }
    }
    // Small batches (a caller that cannot batch: Align = a batch of one): every copy between pageable memory and the
    // device is a staged transfer of 15-25 us, and a call makes 5 of them on the way in and 13 on the way out.  Here
    // the inputs travel as ONE image through the context's pinned buffer and the result arrays come back as one.
    const uint64_t small_img = ((blob_bytes + 15) & ~15ull) + 24 * n_pairs + 64;
    const bool     small     = !sliced && !packed && n_pairs <= 4096 && small_img <= (4u << 20);
    void *d_blob = ctx->in_blob.p, *d_qoff = ctx->in_qoff.p, *d_toff = ctx->in_toff.p, *d_qlen = ctx->in_qlen.p, *d_tlen = ctx->in_tlen.p;
    if (lazy_pack && !sliced) {
        const int e = (*lazy_pack)(0, n_pairs);
        if (e) return e == 2 ? WFAHIP_ERR_UNSUPPORTED : WFAHIP_ERR_HIP;
    }
    if (small) {
        if (!ctx->pin[0]) HIP_TRY(hipHostMalloc(&ctx->pin[0], PIN_CHUNK, hipHostMallocDefault));
        if ((rc = ensure(ctx, ctx->in_small, small_img))) return rc;
        char *const    img = static_cast<char *>(ctx->pin[0]);
        const uint64_t o1 = (blob_bytes + 15) & ~15ull, o2 = o1 + 8 * n_pairs, o3 = o2 + 8 * n_pairs, o4 = o3 + 4 * n_pairs;
        if (blob_bytes) std::memcpy(img, seq_blob, blob_bytes);
        std::memcpy(img + o1, q_off, 8 * n_pairs), std::memcpy(img + o2, t_off, 8 * n_pairs);
        std::memcpy(img + o3, q_len, 4 * n_pairs), std::memcpy(img + o4, t_len, 4 * n_pairs);
        HIP_TRY(hipMemcpyAsync(ctx->in_small.p, img, o4 + 4 * n_pairs, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));  // (the pinned buffer is reused for the results)
        char *const d = static_cast<char *>(ctx->in_small.p);
        d_blob = d, d_qoff = d + o1, d_toff = d + o2, d_qlen = d + o3, d_tlen = d + o4;
    } else {
        if (blob_bytes && !sliced) HIP_TRY(upload_range(0, blob_bytes, st));
        HIP_TRY(hipMemcpyAsync(ctx->in_qoff.p, q_off, n_pairs * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ctx->in_toff.p, t_off, n_pairs * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ctx->in_qlen.p, q_len, n_pairs * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ctx->in_tlen.p, t_len, n_pairs * 4, hipMemcpyHostToDevice, st));
        if (packed) {
            hipLaunchKernelGGL(wfa_scale_offsets_kernel, dim3((uint32_t)((n_pairs + 255) / 256)), dim3(256), 0, st,
                               static_cast<uint64_t *>(ctx->in_qoff.p), static_cast<uint64_t *>(ctx->in_toff.p), n_pairs);
            HIP_TRY(hipGetLastError());
        }
    }

    if (dbg_t) HIP_TRY(hipStreamSynchronize(st));
    const auto t_dev = now();
    // CIGAR ops are merged runs: a first guess of (n+m)/4 + 8 per pair, grown on demand (at most n+m+2 each)
    uint64_t ops_cap = sum_len / 4 + 8 * n_pairs + 1024;
    for (int attempt = 0; attempt < 6; attempt++) {
        if ((rc = ensure(ctx, ctx->out_ops, ops_cap * 8))) return rc;
        uint64_t needed = 0;
        if (sliced && attempt == 0) {
            std::atomic<int> recorded{0}, up_err{0};
            const auto upload_all = [&] {
                if (hipSetDevice(ctx->device) != hipSuccess) up_err = 1;
                for (int k = 0; k < n_sl; k++) {
                    // (host-side packing of slice k runs here, beside the upload of slice k-1 and the alignment of earlier ones)
                    if (!up_err && lazy_pack) {
                        const int e = (*lazy_pack)(sl_first[k], sl_first[k + 1]);
                        if (e) up_err = e == 2 ? 2 : 1;
                    }
                    if (!up_err && sl_hi[k] > sl_lo[k] && upload_range(sl_lo[k], sl_hi[k], ctx->stream_up) != hipSuccess) up_err = 1;
                    if (hipEventRecord(ctx->ev_up[k], ctx->stream_up) != hipSuccess) up_err = 1;
                    recorded = k + 1;
                }
            };
            std::thread uploader;
            try {
                uploader = std::thread(upload_all);
            } catch (...) {  // no thread to be had: upload here, then align (no overlap, same result)
                upload_all();
            }
            wfahip_timing acc{};
            uint64_t      cursor = 0;
            // ---- per-slice assembly (wfa_finalize.hpp) and download beside the next slice's alignment
            const uint64_t n = n_pairs;
            const uint64_t per_blk = (uint64_t)FIN_BLOCK * FIN_ITEMS;
            auto           al8s    = [](uint64_t v) { return (v + 7) & ~7ull; };
            uint64_t       foff    = 0;
            auto           takes   = [&](uint64_t bytes) {
                const uint64_t o = foff;
                foff += al8s(bytes);
                return o;
            };
            const uint64_t so_tot = takes(16 * UP_SLICES), so_blk = takes(8ull * (n / per_blk + UP_SLICES + 1)), so_ooff = takes(8ull * n),
                           so_loc = takes(8ull * n);
            uint64_t so_f[11];
            for (int i = 0; i < 11; i++) so_f[i] = takes(4ull * n);
            const uint64_t so_ops = takes(8ull * ops_cap);
            if ((rc = ensure(ctx, ctx->fin, foff))) {
                if (uploader.joinable()) uploader.join();
                return rc;
            }
            char *const sfb = static_cast<char *>(ctx->fin.p);
            results_zero(out);
            out->n = n;
            bool alloc_ok = true;
            {
                const size_t cnt = std::max<uint64_t>(n, 1);
#define ALLOCS(field, type) alloc_ok = alloc_ok && (out->field = static_cast<type *>(res_alloc(cnt * sizeof(type)))) != nullptr;
                ALLOCS(status, int32_t) ALLOCS(score, uint32_t) ALLOCS(tbegin, int32_t) ALLOCS(tend, int32_t)
                ALLOCS(qbegin, int32_t) ALLOCS(qend, int32_t) ALLOCS(align_len, uint32_t) ALLOCS(matches, uint32_t)
                ALLOCS(gaps, uint32_t) ALLOCS(gap_regions, uint32_t) ALLOCS(ops_off, uint64_t) ALLOCS(ops_len, uint32_t)
#undef ALLOCS
            }
            uint64_t         ops_done = 0, cells_done = 0, host_ops_cap = 0, blk_done = 0;
            uint64_t         deferred_at = ~0ull;  // ops from this offset on did not fit the estimated host array: downloaded at the end
            // one downloader thread takes the slices in order as the main thread marks them ready (state 1 = ready,
            // 2 = nothing to download, skip)
            struct DlTask { uint64_t k0, nk, o0, ops_k; bool with_ops; };
            DlTask           dl_tasks[UP_SLICES] = {};
            std::atomic<int> dl_state[UP_SLICES];
            for (auto &a : dl_state) a = 0;
            std::atomic<int> dl_err{0};
            const auto dl_run = [&] {
                if (hipSetDevice(ctx->device) != hipSuccess) dl_err = 1;
                for (int k = 0; k < n_sl; k++) {
                    while (dl_state[k].load() == 0) std::this_thread::yield();
                    if (dl_state[k].load() == 2 || dl_err) continue;
                    const DlTask t       = dl_tasks[k];
                    void *const dsts[11] = {out->status, out->score, out->tbegin, out->tend, out->qbegin, out->qend,
                                            out->align_len, out->matches, out->gaps, out->gap_regions, out->ops_len};
                    int r2 = WFAHIP_OK;
                    for (int i = 0; i < 11 && r2 == WFAHIP_OK; i++)
                        r2 = download(ctx, static_cast<char *>(dsts[i]) + 4 * t.k0, sfb + so_f[i] + 4 * t.k0, 4ull * t.nk, ctx->stream_dn);
                    if (r2 == WFAHIP_OK) r2 = download(ctx, out->ops_off + t.k0, sfb + so_ooff + 8 * t.k0, 8ull * t.nk, ctx->stream_dn);
                    if (r2 == WFAHIP_OK && t.with_ops) r2 = download(ctx, out->ops + t.o0, sfb + so_ops + 8 * t.o0, 8ull * t.ops_k, ctx->stream_dn);
                    if (r2 != WFAHIP_OK) dl_err = 1;
                }
            };
            std::thread dl_thread;
            bool        dl_inline = false;
            try {
                dl_thread = std::thread(dl_run);
            } catch (...) {
                dl_inline = true;  // no thread: everything is downloaded after the last slice
            }
            const auto dl_finish = [&] {  // slices never marked (early exit) are skipped; then the downloads are waited for / run here
                for (auto &a : dl_state) {
                    int z = 0;
                    a.compare_exchange_strong(z, 2);
                }
                if (dl_thread.joinable()) dl_thread.join();
                else if (dl_inline) dl_run();
            };
            if (!alloc_ok) rc = WFAHIP_ERR_OOM;
            for (int k = 0; k < n_sl && rc == WFAHIP_OK; k++) {
                while (recorded.load() <= k) std::this_thread::yield();  // (the event must have been recorded before the wait)
                if (up_err) {
                    rc = up_err == 2 ? WFAHIP_ERR_UNSUPPORTED : WFAHIP_ERR_HIP;  // (2: a byte outside ACGT -- the caller falls back to the byte path)
                    break;
                }
                if (hipStreamWaitEvent(st, ctx->ev_up[k], 0) != hipSuccess) {
                    rc = WFAHIP_ERR_HIP;
                    break;
                }
                const uint64_t k0 = sl_first[k], nk = sl_first[k + 1] - k0;
                if (nk == 0) {
                    dl_state[k] = 2;
                    continue;
                }
                if (dbg_t) {
                    (void)hipEventSynchronize(ctx->ev_up[k]);
                    std::fprintf(stderr, "[wfahip]   slice %d: blob part here at +%.1f ms\n", k, ms_of(t_dev, now()));
                }
                rc = align_device(ctx, p, ctx->in_blob.p, blob_bytes, static_cast<char *>(ctx->in_qoff.p) + 8 * k0,
                                  static_cast<char *>(ctx->in_qlen.p) + 4 * k0, static_cast<char *>(ctx->in_toff.p) + 8 * k0,
                                  static_cast<char *>(ctx->in_tlen.p) + 4 * k0, nk, max_len,
                                  static_cast<char *>(ctx->out_rec.p) + (size_t)REC_WORDS * 4 * k0, ctx->out_ops.p, ops_cap, &needed, st,
                                  false, cursor);
                cursor = ctx->timing.ops_written;
                acc.kernel_ms += ctx->timing.kernel_ms, acc.total_ms += ctx->timing.total_ms, acc.n_launches += ctx->timing.n_launches;
                acc.n_retried_pairs += ctx->timing.n_retried_pairs, acc.main_kernel_ms += ctx->timing.main_kernel_ms;
                acc.n_main_launches += ctx->timing.n_main_launches, acc.n_packed_pairs += ctx->timing.n_packed_pairs;
                acc.arena_bytes      = std::max(acc.arena_bytes, ctx->timing.arena_bytes);
                acc.main_kernel_kind = ctx->timing.main_kernel_kind;
                if (rc != WFAHIP_OK) break;
                // assemble this slice's part of the result arrays
                const uint32_t nb_k = (uint32_t)((nk + per_blk - 1) / per_blk);
                FinParams F{};
                F.rec = static_cast<const uint32_t *>(ctx->out_rec.p) + (size_t)REC_WORDS * k0;
                F.ops = static_cast<const uint64_t *>(ctx->out_ops.p), F.n = nk;
                F.totals  = reinterpret_cast<unsigned long long *>(sfb + so_tot) + 2 * k;
                F.blk_sum = reinterpret_cast<uint64_t *>(sfb + so_blk) + blk_done;
                F.loc_off = reinterpret_cast<uint64_t *>(sfb + so_loc) + k0;
                F.ops_off = reinterpret_cast<uint64_t *>(sfb + so_ooff) + k0;
                F.status = reinterpret_cast<int32_t *>(sfb + so_f[0]) + k0, F.score = reinterpret_cast<uint32_t *>(sfb + so_f[1]) + k0;
                F.tbegin = reinterpret_cast<int32_t *>(sfb + so_f[2]) + k0, F.tend = reinterpret_cast<int32_t *>(sfb + so_f[3]) + k0;
                F.qbegin = reinterpret_cast<int32_t *>(sfb + so_f[4]) + k0, F.qend = reinterpret_cast<int32_t *>(sfb + so_f[5]) + k0;
                F.align_len = reinterpret_cast<uint32_t *>(sfb + so_f[6]) + k0, F.matches = reinterpret_cast<uint32_t *>(sfb + so_f[7]) + k0;
                F.gaps = reinterpret_cast<uint32_t *>(sfb + so_f[8]) + k0, F.gap_regions = reinterpret_cast<uint32_t *>(sfb + so_f[9]) + k0;
                F.ops_len = reinterpret_cast<uint32_t *>(sfb + so_f[10]) + k0;
                F.ops_out = reinterpret_cast<uint64_t *>(sfb + so_ops) + ops_done, F.ops_base = ops_done;
                bool hip_ok = hipMemsetAsync(F.totals, 0, 16, st) == hipSuccess;
                hipLaunchKernelGGL(fin_scan_blocks, dim3(nb_k), dim3(FIN_BLOCK), 0, st, F);
                hipLaunchKernelGGL(fin_scan_sums, dim3(1), dim3(1024), 0, st, F, nb_k);
                hipLaunchKernelGGL(fin_gather, dim3((uint32_t)((nk + 3) / 4)), dim3(256), 0, st, F);
                hip_ok = hip_ok && hipGetLastError() == hipSuccess &&
                         hipMemcpyAsync(ctx->hpin + HPIN_CTRL + CTRL_WORDS, F.totals, 16, hipMemcpyDeviceToHost, st) == hipSuccess &&
                         hipStreamSynchronize(st) == hipSuccess;
                if (!hip_ok) {
                    rc = WFAHIP_ERR_HIP;
                    break;
                }
                unsigned long long tk[2];
                std::memcpy(tk, ctx->hpin + HPIN_CTRL + CTRL_WORDS, 16);
                const uint64_t ops_k = tk[0];
                cells_done += tk[1], blk_done += nb_k;
                if (!out->ops) {  // size the host op array from the first slice: ops per pair x pairs + 15 %
                    host_ops_cap = std::min<uint64_t>(ops_cap, (uint64_t)((double)ops_k / (double)nk * (double)n * 1.15) + 65536);
                    out->ops     = static_cast<uint64_t *>(res_alloc(std::max<uint64_t>(host_ops_cap, 1) * 8));
                    if (!out->ops) {
                        rc = WFAHIP_ERR_OOM;
                        break;
                    }
                }
                if (deferred_at == ~0ull && ops_done + ops_k > host_ops_cap) deferred_at = ops_done;
                if (dbg_t) std::fprintf(stderr, "[wfahip]   slice %d: aligned + assembled at +%.1f ms\n", k, ms_of(t_dev, now()));
                dl_tasks[k] = DlTask{k0, nk, ops_done, ops_k, deferred_at == ~0ull};
                dl_state[k] = 1;
                ops_done += ops_k;
            }
            if (uploader.joinable()) uploader.join();
            dl_finish();
            if (rc == WFAHIP_OK && dl_err) rc = WFAHIP_ERR_HIP;
            if (rc == WFAHIP_OK || rc == WFAHIP_ERR_OOM) {
                acc.ops_written = ctx->timing.ops_written;
                ctx->timing     = acc;
            }
            if (rc == WFAHIP_ERR_OOM && alloc_ok && needed > ops_cap) {  // the op buffer was too small: the whole blob is resident now, one plain call redoes it
                wfahip_results_free(out);
                HIP_TRY(hipStreamSynchronize(ctx->stream_up));
                ops_cap = std::max(needed, ops_cap) + ops_cap / 2 + 1024;
                continue;
            }
            if (rc == WFAHIP_OK && deferred_at != ~0ull) {  // more ops than estimated: an array of the exact size takes what is there + the rest
                uint64_t *full = static_cast<uint64_t *>(res_alloc(std::max<uint64_t>(ops_done, 1) * 8));
                if (!full) {
                    rc = WFAHIP_ERR_OOM;
                } else {
                    std::memcpy(full, out->ops, deferred_at * 8);
                    res_release(out->ops);
                    out->ops = full;
                    rc = download(ctx, out->ops + deferred_at, sfb + so_ops + 8 * deferred_at, 8ull * (ops_done - deferred_at), st);
                }
            }
            if (rc != WFAHIP_OK) {
                wfahip_results_free(out);
                return rc;
            }
            out->n_ops               = ops_done;
            ctx->timing.cells_stored = cells_done;
            if (dbg_t)
                std::fprintf(stderr, "[wfahip] host entry (sliced): small arrays %.1f ms, upload + alignment + assembly + download %.1f ms\n",
                             ms_of(t_h2d, t_dev), ms_of(t_dev, now()));
            return WFAHIP_OK;
        }
        rc = align_device(ctx, p, d_blob, blob_bytes, d_qoff, d_qlen, d_toff, d_tlen, n_pairs, max_len, ctx->out_rec.p, ctx->out_ops.p,
                          ops_cap, &needed, st, false);
        if (rc == WFAHIP_ERR_OOM && needed > ops_cap) {
            // (with headroom: what a call needs is not the same on every attempt -- a context learns the rows and the window a
            // class of pairs needs while it runs, and the retry passes it takes, each reserving op slots, change with that)
            ops_cap = needed + needed / 3 + 1024;
            continue;
        }
        break;
    }
    if (rc) return rc;

    const auto t_d2h = now();
    // ---- assemble wfahip_results on the device (ops packed in pair order, one array per field), then download
    const uint64_t n         = n_pairs;
    const uint32_t n_blocks  = (uint32_t)((n + (uint64_t)FIN_BLOCK * FIN_ITEMS - 1) / ((uint64_t)FIN_BLOCK * FIN_ITEMS));
    const uint64_t ops_total_cap = std::max<uint64_t>(ctx->timing.ops_written, 1);
    auto           al8       = [](uint64_t v) { return (v + 7) & ~7ull; };
    // layout of ctx->fin (bytes): totals[2] | blk_sum[n_blocks] | ops_off[n] | loc_off[n] | 11 x u32[n] | ops_out
    uint64_t off = 0;
    auto     take = [&](uint64_t bytes) {
        const uint64_t o = off;
        off += al8(bytes);
        return o;
    };
    const uint64_t o_tot = take(16), o_blk = take(8ull * n_blocks), o_ooff = take(8ull * n), o_loc = take(8ull * n);
    uint64_t       o_f[11];
    for (int i = 0; i < 11; i++) o_f[i] = take(4ull * n);
    const uint64_t o_ops = take(8ull * ops_total_cap);
    if ((rc = ensure(ctx, ctx->fin, off))) return rc;
    char *fb = static_cast<char *>(ctx->fin.p);
    FinParams F{};
    F.rec = static_cast<const uint32_t *>(ctx->out_rec.p), F.ops = static_cast<const uint64_t *>(ctx->out_ops.p), F.n = n;
    F.totals  = reinterpret_cast<unsigned long long *>(fb + o_tot);
    F.blk_sum = reinterpret_cast<uint64_t *>(fb + o_blk), F.ops_off = reinterpret_cast<uint64_t *>(fb + o_ooff);
    F.loc_off = reinterpret_cast<uint64_t *>(fb + o_loc);
    F.status = reinterpret_cast<int32_t *>(fb + o_f[0]), F.score = reinterpret_cast<uint32_t *>(fb + o_f[1]);
    F.tbegin = reinterpret_cast<int32_t *>(fb + o_f[2]), F.tend = reinterpret_cast<int32_t *>(fb + o_f[3]);
    F.qbegin = reinterpret_cast<int32_t *>(fb + o_f[4]), F.qend = reinterpret_cast<int32_t *>(fb + o_f[5]);
    F.align_len = reinterpret_cast<uint32_t *>(fb + o_f[6]), F.matches = reinterpret_cast<uint32_t *>(fb + o_f[7]);
    F.gaps = reinterpret_cast<uint32_t *>(fb + o_f[8]), F.gap_regions = reinterpret_cast<uint32_t *>(fb + o_f[9]);
    F.ops_len = reinterpret_cast<uint32_t *>(fb + o_f[10]), F.ops_out = reinterpret_cast<uint64_t *>(fb + o_ops);
    HIP_TRY(hipMemsetAsync(F.totals, 0, 16, st));
    hipLaunchKernelGGL(fin_scan_blocks, dim3(n_blocks), dim3(FIN_BLOCK), 0, st, F);
    hipLaunchKernelGGL(fin_scan_sums, dim3(1), dim3(1024), 0, st, F, n_blocks);
    hipLaunchKernelGGL(fin_gather, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, st, F);
    HIP_TRY(hipGetLastError());
    unsigned long long totals[2] = {0, 0};
    const bool         small_out = small && off <= PIN_CHUNK;  // every result array in ONE copy
    if (small_out) {
        HIP_TRY(hipMemcpyAsync(ctx->pin[0], fb, off, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        std::memcpy(totals, static_cast<char *>(ctx->pin[0]) + o_tot, 16);
    } else {
        HIP_TRY(hipMemcpyAsync(ctx->hpin + HPIN_CTRL + CTRL_WORDS, F.totals, 16, hipMemcpyDeviceToHost, st));  // (pinned)
        HIP_TRY(hipStreamSynchronize(st));
        std::memcpy(totals, ctx->hpin + HPIN_CTRL + CTRL_WORDS, 16);
    }
    const auto t_unp = now();

    results_zero(out);
    out->n = n;
    {
        const size_t cnt = std::max<uint64_t>(n, 1);
#define ALLOC(field, type)                                          \
    out->field = static_cast<type *>(res_alloc(cnt * sizeof(type))); \
    if (!out->field) {                                               \
        wfahip_results_free(out);                                    \
        return WFAHIP_ERR_OOM;                                       \
    }
        ALLOC(status, int32_t) ALLOC(score, uint32_t) ALLOC(tbegin, int32_t) ALLOC(tend, int32_t)
        ALLOC(qbegin, int32_t) ALLOC(qend, int32_t) ALLOC(align_len, uint32_t) ALLOC(matches, uint32_t)
        ALLOC(gaps, uint32_t) ALLOC(gap_regions, uint32_t) ALLOC(ops_off, uint64_t) ALLOC(ops_len, uint32_t)
#undef ALLOC
        out->n_ops = totals[0];
        out->ops   = static_cast<uint64_t *>(res_alloc(std::max<uint64_t>(totals[0], 1) * 8));
        if (!out->ops) {
            wfahip_results_free(out);
            return WFAHIP_ERR_OOM;
        }
    }
    void *const       dsts[11] = {out->status, out->score, out->tbegin, out->tend, out->qbegin, out->qend,
                                  out->align_len, out->matches, out->gaps, out->gap_regions, out->ops_len};
    if (small_out) {
        const char *const img = static_cast<const char *>(ctx->pin[0]);
        for (int i = 0; i < 11; i++) std::memcpy(dsts[i], img + o_f[i], 4ull * n);
        std::memcpy(out->ops_off, img + o_ooff, 8ull * n);
        if (totals[0]) std::memcpy(out->ops, img + o_ops, 8ull * totals[0]);
    } else {
        for (int i = 0; i < 11 && rc == WFAHIP_OK; i++) rc = download(ctx, dsts[i], fb + o_f[i], 4ull * n, st);
        if (rc == WFAHIP_OK) rc = download(ctx, out->ops_off, fb + o_ooff, 8ull * n, st);
        if (rc == WFAHIP_OK) rc = download(ctx, out->ops, fb + o_ops, 8ull * totals[0], st);
    }
    const uint64_t cells = totals[1];
    if (dbg_t)
        std::fprintf(stderr, "[wfahip] host entry: H2D %.1f ms, device %.1f ms, finalize %.1f ms, download %.1f ms\n",
                     ms_of(t_h2d, t_dev), ms_of(t_dev, t_d2h), ms_of(t_d2h, t_unp), ms_of(t_unp, now()));
    ctx->timing.cells_stored = cells;
    if (rc) wfahip_results_free(out);
    return rc;
}

// 16 bases -> one word, eight bytes at a time: the codes are (byte >> 1) & 3, gathered by three shift-or steps; a byte
// outside ACGT shows as a difference between the byte and the canonical letter of its code (0x41 + 2 code, + 15 for T).
namespace {
inline uint32_t pack8(uint64_t w, uint64_t &bad) {
    const uint64_t x = (w >> 1) & 0x0303030303030303ull;
    const uint64_t t = (x >> 1) & ~x & 0x0101010101010101ull;  // code 2 = 'T'
    bad |= (0x4141414141414141ull + 2 * x + 15 * t) ^ w;
    uint64_t y = (x | (x >> 6)) & 0x000F000F000F000Full;
    y          = (y | (y >> 12)) & 0x000000FF000000FFull;
    return (uint32_t)((y | (y >> 24)) & 0xFFFFull);
}
// one sequence -> dst[0 .. (len + 15) / 16] (the last word is the zero pad word); returns true on a byte outside ACGT
bool pack_seq_fast(const uint8_t *s, uint32_t len, uint32_t *dst) {
    uint64_t       bad = 0;
    const uint32_t nw = len / 16;
    for (uint32_t w = 0; w < nw; w++) {
        uint64_t a, b;
        std::memcpy(&a, s + 16 * w, 8), std::memcpy(&b, s + 16 * w + 8, 8);
        dst[w] = pack8(a, bad) | (pack8(b, bad) << 16);
    }
    const uint32_t rem = len - 16 * nw;
    if (rem) {
        uint8_t tail[16];
        std::memset(tail, 'A', 16);
        std::memcpy(tail, s + 16 * nw, rem);
        uint64_t a, b;
        std::memcpy(&a, tail, 8), std::memcpy(&b, tail + 8, 8);
        dst[nw] = pack8(a, bad) | (pack8(b, bad) << 16);
        dst[nw + 1] = 0;
    } else {
        dst[nw] = 0;
    }
    return bad != 0;
}
}  // namespace

// wfahip_align_batch on a large batch: a quarter of the bytes cross PCIe.  The sequences are 2-bit packed by host threads,
// a slice at a time, into a page-locked buffer of the context -- slice k is packed while slice k-1 uploads and earlier
// slices are being aligned -- and expanded again on the device (wfa_unpack_kernel), where bandwidth is free.  A byte outside
// ACGT anywhere (the reference compares raw bytes, wfa.go:408-454) ends the attempt and the batch takes the byte path.
static int align_batch_autopack(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *seq_blob, uint64_t blob_bytes,
                                const uint64_t *q_off, const uint32_t *q_len, const uint64_t *t_off, const uint32_t *t_len,
                                uint64_t n_pairs, wfahip_results *out) {
    if (!ctx || !out || !q_off || !q_len || !t_off || !t_len || !seq_blob) return WFAHIP_ERR_BAD_ARG;
    std::vector<uint64_t> &q_woff = ctx->pack_qw, &t_woff = ctx->pack_tw;  // (kept between calls: fresh pages cost more than the sums)
    q_woff.resize(n_pairs), t_woff.resize(n_pairs);
    uint64_t    pos = 0;
    PackedFacts facts{1u, 0ull};
    for (uint64_t i = 0; i < n_pairs; i++) {
        // (a pair the alignment rejects -- too long, or empty -- is not validated and packs as nothing: exactly the byte entry's rule)
        const bool v = q_len[i] <= WFAHIP_MAX_SEQ_LEN && t_len[i] <= WFAHIP_MAX_SEQ_LEN && q_len[i] && t_len[i];
        if (v && (q_off[i] > blob_bytes || q_len[i] > blob_bytes - q_off[i] || t_off[i] > blob_bytes || t_len[i] > blob_bytes - t_off[i]))
            return WFAHIP_ERR_BAD_ARG;
        if (v) facts.max_len = std::max(facts.max_len, std::max(q_len[i], t_len[i])), facts.sum_len += (uint64_t)q_len[i] + t_len[i];
        q_woff[i] = pos, pos += wfahip_packed_words(v ? q_len[i] : 0);
        t_woff[i] = pos, pos += wfahip_packed_words(v ? t_len[i] : 0);
    }
    // (pairs are packed one by one: a batch whose pairs SHARE sequences -- one target against many queries -- would carry every
    // copy over PCIe; beyond a quarter more than the blob itself the byte path is the cheaper one.  Sharing shows in the BASES
    // the pairs name against the bytes of the blob -- not in the packed words, whose pad word and 16-base rounding per
    // sequence alone are a quarter of a tightly laid-out batch of 100-base reads)
    if (facts.sum_len > blob_bytes + blob_bytes / 4) return WFAHIP_ERR_UNSUPPORTED;
    const size_t need = (size_t)(pos + 4) * 4;
    if (ctx->pack_pin_bytes < need) {
        HIP_TRY(hipSetDevice(ctx->device));
        if (ctx->pack_pin) (void)hipHostFree(ctx->pack_pin);
        ctx->pack_pin = nullptr, ctx->pack_pin_bytes = 0;
        if (hipHostMalloc(reinterpret_cast<void **>(&ctx->pack_pin), need + need / 8, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            ctx->pack_pin = nullptr;
            return WFAHIP_ERR_UNSUPPORTED;  // (no page-locked memory for the packed words: the byte path needs none)
        }
        ctx->pack_pin_bytes = need + need / 8;
    }
    uint32_t *const packed = ctx->pack_pin;
    unsigned n_thr = std::max(1u, std::min(64u, std::thread::hardware_concurrency() / 2));
    if (const char *e = std::getenv("WFAHIP_PACK_THREADS")) n_thr = (unsigned)std::max(1, std::atoi(e));
    const std::function<int(uint64_t, uint64_t)> lazy = [&](uint64_t first, uint64_t last) -> int {
        std::atomic<int> bad{0};
        const auto range = [&](uint64_t a, uint64_t b) {
            bool bd = false;
            for (uint64_t i = a; i < b; i++) {
                if (!(q_len[i] <= WFAHIP_MAX_SEQ_LEN && t_len[i] <= WFAHIP_MAX_SEQ_LEN && q_len[i] && t_len[i])) {
                    packed[q_woff[i]] = 0, packed[t_woff[i]] = 0;
                    continue;
                }
                bd |= pack_seq_fast(seq_blob + q_off[i], q_len[i], packed + q_woff[i]);
                bd |= pack_seq_fast(seq_blob + t_off[i], t_len[i], packed + t_woff[i]);
            }
            if (bd) bad = 1;
        };
        const uint64_t cnt = last - first;
        const unsigned nt  = (unsigned)std::min<uint64_t>(n_thr, cnt / 2048 + 1);
        std::vector<std::thread> th;
        const uint64_t per = (cnt + nt - 1) / nt;
        for (unsigned t = 0; t < nt; t++) {
            const uint64_t a = std::min<uint64_t>(last, first + (uint64_t)t * per), b = std::min<uint64_t>(last, a + per);
            bool inl = nt == 1;
            if (!inl) {
                try {
                    th.emplace_back(range, a, b);
                } catch (...) {
                    inl = true;
                }
            }
            if (inl) range(a, b);
        }
        for (auto &t : th) t.join();
        return bad ? 2 : 0;
    };
    return align_batch_impl(ctx, p, nullptr, pos * 16, q_woff.data(), q_len, t_woff.data(), t_len, n_pairs, out, packed, &lazy, &facts);
}

static int align_batch_entry(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *seq_blob, uint64_t blob_bytes,
                             const uint64_t *q_off, const uint32_t *q_len, const uint64_t *t_off, const uint32_t *t_len,
                             uint64_t n_pairs, wfahip_results *out) {
    if (ctx && out && ctx->opt_autopack != 0 && seq_blob && n_pairs >= 200000 && blob_bytes >= (256u << 20) &&
        !std::getenv("WFAHIP_NO_AUTOPACK") && !std::getenv("WFAHIP_NO_UPLOAD_OVERLAP")) {
        const int rc = align_batch_autopack(ctx, p, seq_blob, blob_bytes, q_off, q_len, t_off, t_len, n_pairs, out);
        if (rc != WFAHIP_ERR_UNSUPPORTED || check_params(p) != WFAHIP_OK) return rc;
        // (a byte outside ACGT somewhere in the batch: the byte path takes all of it)
    }
    return align_batch_impl(ctx, p, seq_blob, blob_bytes, q_off, q_len, t_off, t_len, n_pairs, out);
}

extern "C" int wfahip_align_batch(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *seq_blob,
                                  uint64_t blob_bytes, const uint64_t *q_off, const uint32_t *q_len,
                                  const uint64_t *t_off, const uint32_t *t_len, uint64_t n_pairs,
                                  wfahip_results *out) {
    WFAHIP_GUARD(align_batch_entry(ctx, p, seq_blob, blob_bytes, q_off, q_len, t_off, t_len, n_pairs, out))
}

// ---- score only (wfahip_score_batch): the forward pass without arena or backtrace -- wfa_score_kernel for global pairs, the score
// instances of wfa_wide_kernel for semi-global ones (wfa_score.hip); whatever they hand back goes through the full path above
namespace wfa {
hipError_t wfa_launch_score(const KParams &P, uint32_t grid, size_t lds_bytes, hipStream_t st);
hipError_t wfa_launch_wide_score(int shape, int phase, int waves, const KParams &P, uint32_t grid, size_t lds_bytes, hipStream_t st);
hipError_t wfa_launch_score_long(bool matrix, const KParams &P, uint32_t grid, size_t lds_bytes, hipStream_t st);
hipError_t wfa_launch_score_dev(int k, const SDParams &S, uint32_t grid, hipStream_t st);
}  // namespace wfa

// ---- the pairs of a score batch that wfa_score_long_kernel takes (wfa_score_long.hpp): global pairs with a read beyond wfa_score_kernel's
// SCORE_MAX_LEN, neither empty nor too long.  They are 2-bit packed on host threads into ONE word buffer, in wfahip_pack_pairs' layout
// (pair after pair, query then target, each word-aligned with its pad word), and listed for the kernel: two table entries per pair,
// {word offset lo, hi, length, pair index} for the query and {.., .., length, 0} for the target.  A pair with a byte outside ACGT is
// packed but not listed (`bytes`): it stays on the full path.
namespace {
struct ScoreLongPlan {
    std::vector<uint64_t> ids;     // the long pairs, in batch order
    std::vector<uint64_t> qw, tw;  // word offsets of their sequences
    uint64_t              n_words = 0;
};
void score_long_plan(const uint32_t *q_len, const uint32_t *t_len, uint64_t n_pairs, ScoreLongPlan &pl) {
    for (uint64_t i = 0; i < n_pairs; i++) {
        if (!(q_len[i] && t_len[i] && q_len[i] <= WFAHIP_MAX_SEQ_LEN && t_len[i] <= WFAHIP_MAX_SEQ_LEN)) continue;
        if (std::max(q_len[i], t_len[i]) <= SCORE_MAX_LEN) continue;
        pl.ids.push_back(i);
        pl.qw.push_back(pl.n_words), pl.n_words += wfahip_packed_words(q_len[i]);
        pl.tw.push_back(pl.n_words), pl.n_words += wfahip_packed_words(t_len[i]);
    }
}
// words must hold pl.n_words words
void score_long_pack(const uint8_t *seq_blob, const uint64_t *q_off, const uint32_t *q_len, const uint64_t *t_off, const uint32_t *t_len,
                     const ScoreLongPlan &pl, uint32_t *words, std::vector<uint4> &table, std::vector<uint64_t> &bytes) {
    const uint64_t       n = pl.ids.size();
    std::vector<uint8_t> bad(n, 0);
    const auto           range = [&](uint64_t a, uint64_t b) {
        for (uint64_t j = a; j < b; j++) {
            const uint64_t i = pl.ids[j];
            bool           bd = pack_seq_fast(seq_blob + q_off[i], q_len[i], words + pl.qw[j]);
            bd |= pack_seq_fast(seq_blob + t_off[i], t_len[i], words + pl.tw[j]);
            bad[j] = bd ? 1 : 0;
        }
    };
    unsigned n_thr = std::max(1u, std::min(16u, std::thread::hardware_concurrency() / 2));
    if (const char *e = std::getenv("WFAHIP_PACK_THREADS")) n_thr = (unsigned)std::max(1, std::atoi(e));
    const unsigned           nt = (unsigned)std::min<uint64_t>(std::min<uint64_t>(n_thr, pl.n_words / 65536 + 1), std::max<uint64_t>(n, 1));
    std::vector<std::thread> th;
    const uint64_t           per = (n + nt - 1) / nt;
    for (unsigned t = 0; t < nt; t++) {
        const uint64_t a = std::min<uint64_t>(n, (uint64_t)t * per), b = std::min<uint64_t>(n, a + per);
        bool           inl = nt == 1;
        if (!inl) {
            try {
                th.emplace_back(range, a, b);
            } catch (...) {
                inl = true;
            }
        }
        if (inl) range(a, b);
    }
    for (auto &t : th) t.join();
    table.clear(), bytes.clear();
    for (uint64_t j = 0; j < n; j++) {
        const uint64_t i = pl.ids[j];
        if (bad[j]) {
            bytes.push_back(i);
            continue;
        }
        table.push_back(make_uint4((uint32_t)pl.qw[j], (uint32_t)(pl.qw[j] >> 32), q_len[i], (uint32_t)i));
        table.push_back(make_uint4((uint32_t)pl.tw[j], (uint32_t)(pl.tw[j] >> 32), t_len[i], 0u));
    }
}
}  // namespace

// Debug / test aid, host only: the word buffer and the list above for a batch (include/wfa_hip.h)
extern "C" int wfahip_debug_score_long_list(const uint8_t *seq_blob, const uint64_t *q_off, const uint32_t *q_len, const uint64_t *t_off,
                                            const uint32_t *t_len, uint64_t n_pairs, uint32_t **words, uint64_t *n_words, uint32_t **table,
                                            uint64_t *n_listed) {
    if (!q_off || !q_len || !t_off || !t_len || !words || !n_words || !table || !n_listed || (!seq_blob && n_pairs)) return WFAHIP_ERR_BAD_ARG;
    try {
        ScoreLongPlan pl;
        score_long_plan(q_len, t_len, n_pairs, pl);
        std::vector<uint4>    tb;
        std::vector<uint64_t> bytes;
        uint32_t *const       w = static_cast<uint32_t *>(std::malloc((size_t)(pl.n_words + 1) * 4));
        if (!w) return WFAHIP_ERR_OOM;
        score_long_pack(seq_blob, q_off, q_len, t_off, t_len, pl, w, tb, bytes);
        uint32_t *const t = static_cast<uint32_t *>(std::malloc(tb.size() * 16 + 16));
        if (!t) {
            std::free(w);
            return WFAHIP_ERR_OOM;
        }
        if (!tb.empty()) std::memcpy(t, tb.data(), tb.size() * 16);
        *words = w, *n_words = pl.n_words, *table = t, *n_listed = tb.size() / 2;
        return WFAHIP_OK;
    } catch (const std::bad_alloc &) {
        return WFAHIP_ERR_OOM;
    } catch (...) {
        return WFAHIP_ERR_INTERNAL;
    }
}

extern "C" void wfahip_scores_free(wfahip_scores *s) {
    if (!s) return;
    std::free(s->status), std::free(s->score);
    s->status = nullptr, s->score = nullptr, s->n = 0;
}

// The launch section of a score batch, shared by wfahip_score_batch and wfahip_score_batch_device: P names the batch (device
// pointers), score_out, the penalties and max_score.  LDS sizing from max_len, chunks of 2^24 (global) / 2^18 (semi-global: the wide
// kernel's checkpoints take WIDE_CKPT_WORDS words per pair of a chunk) pairs, the wide kernel's two phases under wf-adaptive, and
// the n_listed pairs of ctx->mx_seq / mx_words on wfa_score_long_kernel behind the short launch.  Records ctx->ev0 before the
// first launch and ctx->ev1 behind the last; synchronises nothing.  n_long: the long pairs of the batch (listed or not).
static int score_launch(wfahip_ctx *ctx, KParams &P, uint64_t n_pairs, uint32_t max_len, int shape, bool skip_short, uint64_t n_listed,
                        uint64_t n_long, hipStream_t st, wfahip_timing &tm, bool &long_main) {
    int            rc;
    const bool     glob = P.global_alignment != 0u;
    const uint32_t L = std::min<uint32_t>(max_len, glob ? SCORE_MAX_LEN : WIDE_MAX_LEN);  // (longer pairs come back ST_REDO_LDS)
    const uint32_t seq_words = (L + 15) / 16 + 1;
    P.lds_seq_words = seq_words;
    // chunks: the wide kernel's checkpoints take WIDE_CKPT_WORDS words per pair of a chunk
    const uint64_t chunk = glob ? (1ull << 24) : (1ull << 18);
    const bool     two_phase = !glob && P.adaptive != 0u;
    if (two_phase && (rc = ensure(ctx, ctx->wide_ckpt, (size_t)std::min<uint64_t>(chunk, n_pairs) * WIDE_CKPT_WORDS * 4))) return rc;
    P.wide_ckpt = static_cast<uint32_t *>(ctx->wide_ckpt.p), P.wide_ckpt_on = two_phase ? 1u : 0u;
    const size_t lds_g = (size_t)score_lds_words(seq_words) * 4;
    const size_t lds_w = (size_t)wide_lds_words(seq_words, L) * 4, lds_n = (size_t)wide_lds_words_narrow(seq_words) * 4;
    const int    waves = lds_w > 12 * 1024 ? 4 : 1;  // (as the full path: rings above 12 KB are shared by four waves)
    P.sub_lds_words = wide_row_hw(L);
    if (!ctx->ev0) HIP_TRY(hipEventCreate(&ctx->ev0));
    if (!ctx->ev1) HIP_TRY(hipEventCreate(&ctx->ev1));
    HIP_TRY(hipEventRecord(ctx->ev0, st));
    for (uint64_t c0 = 0; c0 < n_pairs && !skip_short; c0 += chunk) {
        const uint32_t cn = (uint32_t)std::min<uint64_t>(chunk, n_pairs - c0);
        P.chunk_first = (uint32_t)c0, P.chunk_n = cn;
        if (glob) {
            HIP_TRY(wfa_launch_score(P, cn, lds_g, st));
        } else {
            HIP_TRY(wfa_launch_wide_score(shape, 0, waves, P, cn, lds_w, st));
            if (two_phase) {
                HIP_TRY(wfa_launch_wide_score(shape, 1, 1, P, cn, lds_n, st));
                tm.n_launches++;
            }
        }
        tm.n_launches++, tm.n_main_launches++;
    }
    // the listed long pairs, behind wfa_score_kernel on the same stream: their slots (ST_REDO_LDS there) take the long kernel's result
    long_main = n_listed > n_pairs - n_long;  // it took more pairs of the call than the short kernel
    if (n_listed) {
        KParams PL = P;
        PL.mx_words = static_cast<const uint32_t *>(ctx->mx_words.p);
        PL.lds_seq_words = score_long_window(ctx->opt_score_long_window);
        const size_t lds_l = (size_t)score_long_lds_words(PL.lds_seq_words) * 4;
        for (uint64_t c0 = 0; c0 < n_listed; c0 += chunk) {
            const uint32_t cn = (uint32_t)std::min<uint64_t>(chunk, n_listed - c0);
            PL.mx_seq = static_cast<const uint4 *>(ctx->mx_seq.p) + 2 * c0, PL.chunk_first = 0u, PL.chunk_n = cn;
            HIP_TRY(wfa_launch_score_long(false, PL, cn, lds_l, st));
            tm.n_launches++;
            if (long_main) tm.n_main_launches++;
        }
    }
    HIP_TRY(hipEventRecord(ctx->ev1, st));
    return WFAHIP_OK;
}

static int score_batch_impl(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *seq_blob, uint64_t blob_bytes, const uint64_t *q_off,
                            const uint32_t *q_len, const uint64_t *t_off, const uint32_t *t_len, uint64_t n_pairs, uint32_t max_score,
                            wfahip_scores *out) {
    if (!ctx || !out) return WFAHIP_ERR_BAD_ARG;
    std::memset(out, 0, sizeof *out);
    int rc = check_params(p);
    if (rc) return rc;
    if (n_pairs == 0) return WFAHIP_OK;
    if (!q_off || !q_len || !t_off || !t_len || (!seq_blob && blob_bytes)) return WFAHIP_ERR_BAD_ARG;
    // the checks of align_batch_impl: every pair that is neither empty nor too long lies inside the blob
    uint32_t max_len = 1;
    for (uint64_t i = 0; i < n_pairs; i++) {
        if (q_len[i] <= WFAHIP_MAX_SEQ_LEN && t_len[i] <= WFAHIP_MAX_SEQ_LEN && q_len[i] && t_len[i]) {
            if (q_off[i] > blob_bytes || q_len[i] > blob_bytes - q_off[i] || t_off[i] > blob_bytes || t_len[i] > blob_bytes - t_off[i])
                return WFAHIP_ERR_BAD_ARG;
            max_len = std::max(max_len, std::max(q_len[i], t_len[i]));
        }
    }
    HIP_TRY(hipSetDevice(ctx->device));
    const auto t_start = std::chrono::steady_clock::now();
    std::vector<uint2> res(n_pairs);
    wfahip_timing      tm{};

    KParams P{};
    P.x = p->mismatch, P.o = p->gap_open, P.e = p->gap_ext, P.oe = p->gap_open + p->gap_ext;
    P.g = gcd_u32(gcd_u32(P.x, P.oe), P.e);
    P.global_alignment = p->global_alignment ? 1u : 0u, P.adaptive = p->adaptive ? 1u : 0u;
    P.min_wf_len = p->min_wf_len, P.max_dist_diff = p->max_dist_diff;
    const uint32_t dx = P.x / P.g, doe = P.oe / P.g, de = P.e / P.g;
    const bool     glob  = P.global_alignment != 0u;
    const int      shape = fwd_shape(dx, doe, de);
    const bool     on_kernel = glob ? score_shape_ok(dx, doe, de) : shape >= 0;
    // ---- global pairs beyond wfa_score_kernel's length: wfa_score_long_kernel takes them when the call holds at least "score_long_min"
    // of them; they are packed here (host threads) into the context's page-locked word buffer and listed
    ScoreLongPlan         lp;
    std::vector<uint4>    ltab;    // two entries per listed pair
    std::vector<uint64_t> lbytes;  // long pairs with a byte outside ACGT: the full path
    bool                  use_long = false;
    if (on_kernel && glob && n_pairs <= UINT32_MAX) {
        score_long_plan(q_len, t_len, n_pairs, lp);
        use_long = !lp.ids.empty() && (int64_t)lp.ids.size() >= ctx->opt_score_long_min;
    }
    if (use_long) {
        const size_t need = (size_t)(lp.n_words + 4) * 4;
        if (ctx->pack_pin_bytes < need) {
            if (ctx->pack_pin) (void)hipHostFree(ctx->pack_pin);
            ctx->pack_pin = nullptr, ctx->pack_pin_bytes = 0;
            if (hipHostMalloc(reinterpret_cast<void **>(&ctx->pack_pin), need + need / 8, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                ctx->pack_pin = nullptr;
                use_long = false;  // (no page-locked memory for the words: these pairs take the full path, as below the gate)
            } else {
                ctx->pack_pin_bytes = need + need / 8;
            }
        }
    }
    if (use_long) score_long_pack(seq_blob, q_off, q_len, t_off, t_len, lp, ctx->pack_pin, ltab, lbytes);
    const uint64_t n_listed   = ltab.size() / 2;
    const bool     skip_short = use_long && lp.ids.size() == n_pairs;  // every pair is long: nothing for wfa_score_kernel
    if (on_kernel) {
        hipStream_t st = ctx->stream;
        if ((rc = ensure(ctx, ctx->score_out, n_pairs * 8))) return rc;
        if (!skip_short) {
            if ((rc = ensure(ctx, ctx->in_blob, blob_bytes + 32))) return rc;
            if ((rc = ensure(ctx, ctx->in_qoff, n_pairs * 8))) return rc;
            if ((rc = ensure(ctx, ctx->in_toff, n_pairs * 8))) return rc;
            if ((rc = ensure(ctx, ctx->in_qlen, n_pairs * 4))) return rc;
            if ((rc = ensure(ctx, ctx->in_tlen, n_pairs * 4))) return rc;
            if (blob_bytes) HIP_TRY(hipMemcpyAsync(ctx->in_blob.p, seq_blob, blob_bytes, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(ctx->in_qoff.p, q_off, n_pairs * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(ctx->in_toff.p, t_off, n_pairs * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(ctx->in_qlen.p, q_len, n_pairs * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(ctx->in_tlen.p, t_len, n_pairs * 4, hipMemcpyHostToDevice, st));
        }
        if (n_listed) {
            if ((rc = ensure(ctx, ctx->mx_seq, ltab.size() * 16))) return rc;
            if ((rc = ensure(ctx, ctx->mx_words, (size_t)(lp.n_words + 4) * 4))) return rc;
            HIP_TRY(hipMemcpyAsync(ctx->mx_seq.p, ltab.data(), ltab.size() * 16, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(ctx->mx_words.p, ctx->pack_pin, (size_t)lp.n_words * 4, hipMemcpyHostToDevice, st));
        }
        P.blob = static_cast<const uint8_t *>(ctx->in_blob.p), P.blob_bytes = blob_bytes;
        P.q_off = static_cast<const uint64_t *>(ctx->in_qoff.p), P.t_off = static_cast<const uint64_t *>(ctx->in_toff.p);
        P.q_len = static_cast<const uint32_t *>(ctx->in_qlen.p), P.t_len = static_cast<const uint32_t *>(ctx->in_tlen.p);
        P.score_out = static_cast<uint2 *>(ctx->score_out.p), P.max_score = max_score;
        P.dx = dx, P.doe = doe, P.de = de, P.census = 0u, P.wide_exact = 0u, P.work = nullptr;
        bool long_main = false;
        if ((rc = score_launch(ctx, P, n_pairs, max_len, shape, skip_short, n_listed, lp.ids.size(), st, tm, long_main))) return rc;
        HIP_TRY(hipMemcpyAsync(res.data(), ctx->score_out.p, n_pairs * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        tm.kernel_ms = tm.main_kernel_ms = ms;
        tm.main_kernel_kind = glob ? (long_main ? 23u : 19u) : 20u;
        // (long pairs that were not listed: wfa_score_kernel said ST_REDO_LDS, or never saw them)
        for (const uint64_t i : lbytes) res[i] = make_uint2(ST_REDO_BYTES, 0u);
    } else {
        for (uint64_t i = 0; i < n_pairs; i++) res[i] = make_uint2(ST_REDO_BAND, 0u);
    }
    // what the kernels handed back (bytes outside ACGT, a band or a length they cannot hold, a shape without an instance): the full path
    std::vector<uint64_t> fb;
    for (uint64_t i = 0; i < n_pairs; i++)
        if (res[i].x >= ST_REDO_BYTES) fb.push_back(i);
    if (!fb.empty()) {
        std::vector<uint64_t> qo(fb.size()), to(fb.size());
        std::vector<uint32_t> ql(fb.size()), tl(fb.size());
        for (size_t j = 0; j < fb.size(); j++) qo[j] = q_off[fb[j]], to[j] = t_off[fb[j]], ql[j] = q_len[fb[j]], tl[j] = t_len[fb[j]];
        wfahip_results r;
        if ((rc = align_batch_entry(ctx, p, seq_blob, blob_bytes, qo.data(), ql.data(), to.data(), tl.data(), fb.size(), &r))) return rc;
        for (size_t j = 0; j < fb.size(); j++) {
            const uint32_t st = (uint32_t)r.status[j], sc = r.score[j];
            res[fb[j]] = (st == ST_OK && max_score != 0u && sc > max_score) ? make_uint2(ST_OVER_MAX, 0u) : make_uint2(st, sc);
        }
        wfahip_results_free(&r);
        const wfahip_timing &f = ctx->timing;
        tm.kernel_ms += f.kernel_ms, tm.n_launches += f.n_launches, tm.arena_bytes = f.arena_bytes;
        if (!on_kernel) tm.main_kernel_ms = f.main_kernel_ms, tm.n_main_launches = f.n_main_launches, tm.main_kernel_kind = f.main_kernel_kind;
    }
    tm.n_retried_pairs = (uint32_t)fb.size();
    out->status = static_cast<int32_t *>(std::malloc(n_pairs * 4));
    out->score  = static_cast<uint32_t *>(std::malloc(n_pairs * 4));
    if (!out->status || !out->score) {
        wfahip_scores_free(out);
        return WFAHIP_ERR_OOM;
    }
    out->n = n_pairs;
    for (uint64_t i = 0; i < n_pairs; i++) out->status[i] = (int32_t)res[i].x, out->score[i] = res[i].x == ST_OK ? res[i].y : 0u;
    tm.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    ctx->timing = tm;
    return WFAHIP_OK;
}

extern "C" int wfahip_score_batch(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *seq_blob, uint64_t blob_bytes, const uint64_t *q_off,
                                  const uint32_t *q_len, const uint64_t *t_off, const uint32_t *t_len, uint64_t n_pairs, uint32_t max_score,
                                  wfahip_scores *out) {
    WFAHIP_GUARD(score_batch_impl(ctx, p, seq_blob, blob_bytes, q_off, q_len, t_off, t_len, n_pairs, max_score, out))
}

// ---- score only on device-resident input (wfahip_score_batch_device): score_batch_impl with everything it does on the host done by
// the kernels of wfa_score_dev.hpp.  The host sees three blocks of SDC_WORDS counters -- after the plan (bounds flag, longest
// length, long pairs, their words), after the list (listed pairs) when long pairs run, after the redo count (pairs of the full path,
// their bases, their longest length) -- and nothing else of the batch.
namespace {
constexpr uint64_t SD_FB_PAIRS = 1ull << 20;  // pairs per call of the full path: 64 MB of records
}

static int score_batch_device_impl(wfahip_ctx *ctx, const wfahip_params *p, const void *d_blob, uint64_t blob_bytes, const void *d_q_off,
                                   const void *d_q_len, const void *d_t_off, const void *d_t_len, uint64_t n_pairs, uint32_t max_len,
                                   uint32_t max_score, void *d_status, void *d_score, hipStream_t st) {
    if (!ctx || !p) return WFAHIP_ERR_BAD_ARG;
    if (n_pairs && (!d_q_off || !d_q_len || !d_t_off || !d_t_len || !d_status || !d_score || (!d_blob && blob_bytes))) return WFAHIP_ERR_BAD_ARG;
    int rc = check_params(p);
    if (rc) return rc;
    if (n_pairs == 0) return WFAHIP_OK;
    if (n_pairs > 0xFFFFFFF0ull) return WFAHIP_ERR_BAD_ARG;  // (align_device's limit: pair indices are 32-bit on the device)
    HIP_TRY(hipSetDevice(ctx->device));
    if (!st) st = ctx->stream;
    const auto    t_start = std::chrono::steady_clock::now();
    wfahip_timing tm{};
    ctx->sd_n_words = ctx->sd_n_listed = 0;

    KParams P{};
    P.x = p->mismatch, P.o = p->gap_open, P.e = p->gap_ext, P.oe = p->gap_open + p->gap_ext;
    P.g = gcd_u32(gcd_u32(P.x, P.oe), P.e);
    P.global_alignment = p->global_alignment ? 1u : 0u, P.adaptive = p->adaptive ? 1u : 0u;
    P.min_wf_len = p->min_wf_len, P.max_dist_diff = p->max_dist_diff;
    const uint32_t dx = P.x / P.g, doe = P.oe / P.g, de = P.e / P.g;
    const bool     glob  = P.global_alignment != 0u;
    const int      shape = fwd_shape(dx, doe, de);
    const bool     on_kernel = glob ? score_shape_ok(dx, doe, de) : shape >= 0;

    const uint64_t n_tiles = (n_pairs + SD_TILE - 1) / SD_TILE;
    if ((rc = ensure(ctx, ctx->sd_ctl, SDC_WORDS * 8))) return rc;
    if ((rc = ensure(ctx, ctx->sd_blk, n_tiles * sizeof(SDSum)))) return rc;
    SDParams S{};
    S.blob = static_cast<const uint8_t *>(d_blob), S.blob_bytes = blob_bytes;
    S.q_off = static_cast<const uint64_t *>(d_q_off), S.t_off = static_cast<const uint64_t *>(d_t_off);
    S.q_len = static_cast<const uint32_t *>(d_q_len), S.t_len = static_cast<const uint32_t *>(d_t_len);
    S.ctl = static_cast<unsigned long long *>(ctx->sd_ctl.p), S.blk = static_cast<SDSum *>(ctx->sd_blk.p);
    S.d_status = static_cast<int32_t *>(d_status), S.d_score = static_cast<uint32_t *>(d_score), S.max_score = max_score;
    // a selection's count launch over `items` items and the scan of its tile sums into control words c_cnt / c_wt
    const auto count_and_scan = [&](int k, uint64_t items, uint32_t c_cnt, uint32_t c_wt) -> int {
        const uint64_t tiles = (items + SD_TILE - 1) / SD_TILE;
        SDParams       T = S;
        T.n = items;
        HIP_TRY(wfa_launch_score_dev(k, T, (uint32_t)tiles, st));
        T.n = tiles, T.c_cnt = c_cnt, T.c_wt = c_wt;
        HIP_TRY(wfa_launch_score_dev(SDK_SCAN, T, 1, st));
        return WFAHIP_OK;
    };
    const auto launch = [&](int k, uint64_t items, uint64_t per_group) -> int {
        SDParams T = S;
        T.n = items;
        HIP_TRY(wfa_launch_score_dev(k, T, (uint32_t)((items + per_group - 1) / per_group), st));
        return WFAHIP_OK;
    };
    uint64_t   hc[SDC_WORDS];
    const auto fetch_ctl = [&]() -> int {  // (through the context's pinned block: a pageable copy of 64 bytes costs 0.3 ms)
        HIP_TRY(hipMemcpyAsync(ctx->hpin + HPIN_CTRL, S.ctl, SDC_WORDS * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        std::memcpy(hc, ctx->hpin + HPIN_CTRL, SDC_WORDS * 8);
        return WFAHIP_OK;
    };
    static_assert(SDC_WORDS * 8 <= HPIN_REDO * 4, "the control words fit the head of the pinned block");

    // ---- plan: bounds, the longest length, the long pairs.  No kernel that reads a sequence byte runs before its verdict is in
    HIP_TRY(hipMemsetAsync(S.ctl, 0, SDC_WORDS * 8, st));
    S.want_long = (on_kernel && glob) ? 1u : 0u;
    if ((rc = count_and_scan(SDK_PLAN_COUNT, n_pairs, SDC_N_LONG, SDC_N_WORDS))) return rc;
    if ((rc = fetch_ctl())) return rc;
    if (hc[SDC_BOUNDS] != 0) return WFAHIP_ERR_BAD_ARG;
    if (max_len == 0) max_len = (uint32_t)std::max<uint64_t>(1, hc[SDC_MAX_LEN]);
    const uint64_t n_long = hc[SDC_N_LONG], n_words = hc[SDC_N_WORDS];
    const bool     use_long = n_long != 0 && (int64_t)n_long >= ctx->opt_score_long_min;
    uint64_t       n_listed = 0;
    if (on_kernel && (rc = ensure(ctx, ctx->score_out, n_pairs * 8))) return rc;
    S.score_out = static_cast<uint2 *>(ctx->score_out.p);
    if (use_long) {
        // ---- the long pairs: listed (plan, write launch), packed from the caller's blob, and those without a byte outside ACGT tabled
        if ((rc = ensure(ctx, ctx->sd_list, n_long * 24))) return rc;
        if ((rc = ensure(ctx, ctx->mx_seq, n_long * 32))) return rc;
        if ((rc = ensure(ctx, ctx->mx_words, (size_t)(n_words + 4) * 4))) return rc;
        S.l_qw = static_cast<uint64_t *>(ctx->sd_list.p), S.l_tw = S.l_qw + n_long;
        S.l_id = reinterpret_cast<uint32_t *>(S.l_tw + n_long), S.l_bad = S.l_id + n_long;
        S.words = static_cast<uint32_t *>(ctx->mx_words.p), S.table = static_cast<uint4 *>(ctx->mx_seq.p);
        if ((rc = launch(SDK_PLAN_WRITE, n_pairs, SD_TILE))) return rc;
        {
            SDParams T = S;
            T.n = n_long;
            HIP_TRY(wfa_launch_score_dev(SDK_PACK, T, (uint32_t)std::min<uint64_t>(2 * n_long, 1u << 20), st));
        }
        if ((rc = count_and_scan(SDK_LIST_COUNT, n_long, SDC_N_LISTED, SDC_N_REDO))) return rc;  // (no weights: the second total is 0)
        if ((rc = launch(SDK_LIST_WRITE, n_long, SD_TILE))) return rc;
        if ((rc = fetch_ctl())) return rc;
        n_listed = hc[SDC_N_LISTED];
        ctx->sd_n_words = n_words, ctx->sd_n_listed = n_listed;
    }
    // ---- the score kernels, as wfahip_score_batch launches them
    if (on_kernel) {
        const bool skip_short = use_long && n_long == n_pairs;
        P.blob = S.blob, P.blob_bytes = blob_bytes, P.q_off = S.q_off, P.t_off = S.t_off, P.q_len = S.q_len, P.t_len = S.t_len;
        P.score_out = S.score_out, P.max_score = max_score;
        P.dx = dx, P.doe = doe, P.de = de, P.census = 0u, P.wide_exact = 0u, P.work = nullptr;
        bool long_main = false;
        if ((rc = score_launch(ctx, P, n_pairs, max_len, shape, skip_short, n_listed, use_long ? n_long : 0, st, tm, long_main))) return rc;
        tm.main_kernel_kind = glob ? (long_main ? 23u : 19u) : 20u;
    }
    // ---- what they handed back (every pair, for a shape without an instance): counted, then gathered in pair order
    S.all = on_kernel ? 0u : 1u;
    if ((rc = count_and_scan(SDK_REDO_COUNT, n_pairs, SDC_N_REDO, SDC_REDO_SUM))) return rc;
    if (on_kernel && (rc = launch(SDK_FINISH, n_pairs, SD_BLOCK))) return rc;
    if ((rc = fetch_ctl())) return rc;
    if (on_kernel) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        tm.kernel_ms = tm.main_kernel_ms = ms;
    }
    const uint64_t n_redo = hc[SDC_N_REDO], sum_len = hc[SDC_REDO_SUM];
    const uint32_t fb_max = (uint32_t)std::max<uint64_t>(1, hc[SDC_REDO_MAX]);
    if (n_redo) {
        if ((rc = ensure(ctx, ctx->sd_redo, n_redo * 28))) return rc;
        S.r_qoff = static_cast<uint64_t *>(ctx->sd_redo.p), S.r_toff = S.r_qoff + n_redo;
        S.r_id = reinterpret_cast<uint32_t *>(S.r_toff + n_redo), S.r_qlen = S.r_id + n_redo, S.r_tlen = S.r_qlen + n_redo;
        if ((rc = launch(SDK_REDO_WRITE, n_pairs, SD_TILE))) return rc;
        for (uint64_t a = 0; a < n_redo; a += SD_FB_PAIRS) {
            const uint64_t nb = std::min(SD_FB_PAIRS, n_redo - a);
            if ((rc = ensure(ctx, ctx->out_rec, nb * REC_WORDS * 4))) return rc;
            // CIGAR ops are merged runs: the host entry's first guess, (n+m)/4 + 8 per pair, run again once with what was needed
            uint64_t ops_cap = std::min<uint64_t>(sum_len, 2ull * fb_max * nb) / 4 + 8 * nb + 1024;
            for (int attempt = 0;; attempt++) {
                if ((rc = ensure(ctx, ctx->out_ops, ops_cap * 8))) return rc;
                uint64_t needed = 0;
                rc = align_device(ctx, p, d_blob, blob_bytes, S.r_qoff + a, S.r_qlen + a, S.r_toff + a, S.r_tlen + a, nb, fb_max, ctx->out_rec.p,
                                  ctx->out_ops.p, ops_cap, &needed, st, false);
                if (rc == WFAHIP_ERR_OOM && needed > ops_cap && attempt == 0) {
                    ops_cap = needed;
                    continue;
                }
                break;
            }
            if (rc) return rc;
            const wfahip_timing &f = ctx->timing;
            tm.kernel_ms += f.kernel_ms, tm.n_launches += f.n_launches, tm.arena_bytes = std::max(tm.arena_bytes, f.arena_bytes);
            if (!on_kernel && a == 0) tm.main_kernel_ms = f.main_kernel_ms, tm.n_main_launches = f.n_main_launches, tm.main_kernel_kind = f.main_kernel_kind;
            SDParams T = S;
            T.n = nb, T.first = a, T.rec = static_cast<const uint32_t *>(ctx->out_rec.p);
            HIP_TRY(wfa_launch_score_dev(SDK_FINISH, T, (uint32_t)((nb + SD_BLOCK - 1) / SD_BLOCK), st));
        }
        HIP_TRY(hipStreamSynchronize(st));
    }
    tm.n_retried_pairs = (uint32_t)std::min<uint64_t>(n_redo, UINT32_MAX);
    tm.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    ctx->timing = tm;
    return WFAHIP_OK;
}

extern "C" int wfahip_score_batch_device(wfahip_ctx *ctx, const wfahip_params *p, const void *d_seq_blob, uint64_t blob_bytes,
                                         const void *d_q_off, const void *d_q_len, const void *d_t_off, const void *d_t_len,
                                         uint64_t n_pairs, uint32_t max_len, uint32_t max_score, void *d_status, void *d_score, void *stream) {
    WFAHIP_GUARD(score_batch_device_impl(ctx, p, d_seq_blob, blob_bytes, d_q_off, d_q_len, d_t_off, d_t_len, n_pairs, max_len, max_score, d_status,
                                         d_score, static_cast<hipStream_t>(stream)))
}

// Debug / test aid: the packed words and the table the last wfahip_score_batch_device call on ctx handed wfa_score_long_kernel
// (include/wfa_hip.h), copied to the host
extern "C" int wfahip_debug_score_device_list(wfahip_ctx *ctx, uint32_t **words, uint64_t *n_words, uint32_t **table, uint64_t *n_listed) {
    if (!ctx || !words || !n_words || !table || !n_listed) return WFAHIP_ERR_BAD_ARG;
    *words = *table = nullptr, *n_words = *n_listed = 0;
    const uint64_t nw = ctx->sd_n_words, nl = ctx->sd_n_listed;
    if (nw == 0) return WFAHIP_OK;
    if (ctx->mx_words.bytes < nw * 4 || ctx->mx_seq.bytes < nl * 32) return WFAHIP_ERR_INTERNAL;
    HIP_TRY(hipSetDevice(ctx->device));
    uint32_t *const w = static_cast<uint32_t *>(std::malloc((size_t)nw * 4 + 4)), *const t = static_cast<uint32_t *>(std::malloc((size_t)nl * 32 + 16));
    if (!w || !t) {
        std::free(w), std::free(t);
        return WFAHIP_ERR_OOM;
    }
    if (hipMemcpy(w, ctx->mx_words.p, (size_t)nw * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        (nl && hipMemcpy(t, ctx->mx_seq.p, (size_t)nl * 32, hipMemcpyDeviceToHost) != hipSuccess)) {
        std::free(w), std::free(t);
        return WFAHIP_ERR_HIP;
    }
    *words = w, *n_words = nw, *table = t, *n_listed = nl;
    return WFAHIP_OK;
}

// ---- score matrix (wfahip_score_matrix): every query against every target, score only.  The n_q + n_t sequences are packed and
// flagged once (host threads, pack_seq_fast) and uploaded as one table of 2-bit words; the matrix instances of the score kernels
// take the cells of a rectangular tile, a workgroup per cell, and stage the cell's two sequences from the table.  Tiles are
// double-buffered: tile c downloads on stream2 while tile c + 1 runs, and the host scatters it into the caller's arrays.  What the
// kernels hand back goes through the full path of wfahip_align_batch, in batches of MX_FB_PAIRS cells.
namespace wfa {
hipError_t wfa_launch_score_matrix(const KParams &P, uint32_t grid, size_t lds_bytes, hipStream_t st);
hipError_t wfa_launch_wide_score_matrix(int shape, int phase, int waves, const KParams &P, uint32_t grid, size_t lds_bytes, hipStream_t st);
}  // namespace wfa

namespace {
constexpr uint64_t MX_TILE_GLOBAL = 1ull << 22;  // cells per tile of wfa_score_kernel<true>: 32 MB of {status, score}
constexpr uint64_t MX_CKPT_BYTES  = 1ull << 30;  // the wide kernel's checkpoints of one tile (WIDE_CKPT_WORDS words per cell in flight)
constexpr uint64_t MX_FB_PAIRS    = 1ull << 16;  // cells per call of the full path
}  // namespace

static int score_matrix_impl(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *seq_blob, uint64_t blob_bytes, const uint64_t *q_off,
                             const uint32_t *q_len, uint64_t n_q, const uint64_t *t_off, const uint32_t *t_len, uint64_t n_t, uint32_t max_score,
                             int32_t *status, uint32_t *score, uint64_t out_stride) {
    // (every check before any device work, and none dereferences ctx)
    if (!ctx || !p || !status || !score) return WFAHIP_ERR_BAD_ARG;
    if ((n_q && (!q_off || !q_len)) || (n_t && (!t_off || !t_len)) || (!seq_blob && blob_bytes)) return WFAHIP_ERR_BAD_ARG;
    const auto outside = [&](const uint64_t *off, const uint32_t *len, uint64_t n) {  // align_batch_impl's rule, per sequence
        for (uint64_t i = 0; i < n; i++)
            if (len[i] && len[i] <= WFAHIP_MAX_SEQ_LEN && (off[i] > blob_bytes || len[i] > blob_bytes - off[i])) return true;
        return false;
    };
    if (outside(q_off, q_len, n_q) || outside(t_off, t_len, n_t)) return WFAHIP_ERR_BAD_ARG;
    const uint64_t stride = out_stride ? out_stride : n_t;
    if (out_stride && out_stride < n_t) return WFAHIP_ERR_BAD_ARG;
    if (n_q > 1 && stride && n_q - 1 > (UINT64_MAX - n_t) / stride) return WFAHIP_ERR_BAD_ARG;  // (n_q - 1) * stride + n_t overflows
    int rc = check_params(p);
    if (rc) return rc;
    if (n_q == 0 || n_t == 0) return WFAHIP_OK;

    HIP_TRY(hipSetDevice(ctx->device));
    const auto    t_start = std::chrono::steady_clock::now();
    wfahip_timing tm{};
    const auto    put = [&](uint64_t i, uint64_t j, uint32_t st, uint32_t sc) {
        status[i * stride + j] = (int32_t)st, score[i * stride + j] = st == ST_OK ? sc : 0u;
    };
    KParams P{};
    P.x = p->mismatch, P.o = p->gap_open, P.e = p->gap_ext, P.oe = p->gap_open + p->gap_ext;
    P.g = gcd_u32(gcd_u32(P.x, P.oe), P.e);
    P.global_alignment = p->global_alignment ? 1u : 0u, P.adaptive = p->adaptive ? 1u : 0u;
    P.min_wf_len = p->min_wf_len, P.max_dist_diff = p->max_dist_diff;
    const uint32_t dx = P.x / P.g, doe = P.oe / P.g, de = P.e / P.g;
    const bool     glob      = P.global_alignment != 0u;
    const int      shape     = fwd_shape(dx, doe, de);
    const bool     on_kernel = glob ? score_shape_ok(dx, doe, de) : shape >= 0;
    std::vector<uint64_t> fb;  // cells (i * n_t + j) the kernels handed back
    if (on_kernel) {
        hipStream_t st = ctx->stream, st_dn = ctx->stream2;
        // ---- the sequence table: queries, then targets (none when they are the queries)
        const bool     same  = q_off == t_off && q_len == t_len && n_q == n_t;
        const uint64_t n_seq = same ? n_q : n_q + n_t;
        const uint32_t kmax  = glob ? SCORE_MAX_LEN : WIDE_MAX_LEN;
        std::vector<uint4> seq(n_seq);
        uint64_t           pos = 0;
        uint32_t           L   = 1;
        const auto flag_of = [&](uint64_t s) {
            const uint32_t len = s < n_q ? q_len[s] : t_len[s - n_q];
            return len == 0 ? (uint32_t)MXF_EMPTY : len > WFAHIP_MAX_SEQ_LEN ? (uint32_t)MXF_TOO_LONG : len > kmax ? (uint32_t)MXF_LONG : 0u;
        };
        // cells of the global matrix with a long sequence and nothing else against them (flags MXF_LONG only) run on wfa_score_long_kernel when
        // the call holds at least "score_long_min" of them: the long sequences are then packed into the table too.  Counted from the flags of
        // the two sides: {sequences without a flag, sequences flagged `want` only}
        const auto count_side = [&](uint64_t a, uint64_t b, const auto &fl, uint64_t &plain, uint64_t &lng) {
            plain = lng = 0;
            for (uint64_t s = a; s < b; s++) {
                const uint32_t f = fl(s);
                plain += f == 0u, lng += f == MXF_LONG;
            }
        };
        const auto long_cells = [&](const auto &fl) {
            uint64_t pq, lq_, pt, lt_;
            count_side(0, n_q, fl, pq, lq_);
            if (same) pt = pq, lt_ = lq_;
            else count_side(n_q, n_seq, fl, pt, lt_);
            return lq_ * (pt + lt_) + pq * lt_;
        };
        bool use_long = glob && long_cells(flag_of) >= (uint64_t)ctx->opt_score_long_min;
        for (uint64_t s = 0; s < n_seq; s++) {
            const uint32_t len  = s < n_q ? q_len[s] : t_len[s - n_q];
            const uint32_t flag = flag_of(s);
            seq[s] = make_uint4((uint32_t)pos, (uint32_t)(pos >> 32), len, flag);
            if (flag == 0u) L = std::max(L, len);
            if (flag == 0u || (use_long && flag == MXF_LONG)) pos += wfahip_packed_words(len);
        }
        std::vector<uint32_t> words(pos + 4);
        {
            const auto range = [&](uint64_t a, uint64_t b) {
                for (uint64_t s = a; s < b; s++) {
                    if (!(seq[s].w == 0u || (use_long && seq[s].w == MXF_LONG))) continue;
                    const uint8_t *src = seq_blob + (s < n_q ? q_off[s] : t_off[s - n_q]);
                    if (pack_seq_fast(src, seq[s].z, words.data() + ((uint64_t)seq[s].y << 32 | seq[s].x))) seq[s].w |= MXF_BYTES;
                }
            };
            const unsigned nt = (unsigned)std::min<uint64_t>(std::max(1u, std::min(16u, std::thread::hardware_concurrency() / 2)), n_seq / 4096 + 1);
            std::vector<std::thread> th;
            const uint64_t           per = (n_seq + nt - 1) / nt;
            for (unsigned t = 0; t < nt; t++) {
                const uint64_t a = std::min<uint64_t>(n_seq, (uint64_t)t * per), b = std::min<uint64_t>(n_seq, a + per);
                bool inl = nt == 1;
                if (!inl) {
                    try {
                        th.emplace_back(range, a, b);
                    } catch (...) {
                        inl = true;
                    }
                }
                if (inl) range(a, b);
            }
            for (auto &t : th) t.join();
        }
        // (the count again, now that the bytes are known: cells with a byte outside ACGT stay on the full path and do not open the gate)
        uint64_t n_long_cells = 0;
        if (use_long) {
            n_long_cells = long_cells([&](uint64_t s) { return seq[s].w; });
            use_long     = n_long_cells >= (uint64_t)ctx->opt_score_long_min;
        }
        // sequences flagged MXF_LONG before each index: a tile has a cell for the long kernel when a row or a column of it is long, and none
        // for wfa_score_kernel<MATRIX> when all its rows or all its columns are
        std::vector<uint64_t> n_lng(use_long ? n_seq + 1 : 0, 0);
        for (uint64_t s = 0; s < n_seq && use_long; s++) n_lng[s + 1] = n_lng[s] + ((seq[s].w & MXF_LONG) ? 1u : 0u);
        const bool long_main = use_long && n_long_cells > n_q * n_t - n_long_cells;
        if ((rc = ensure(ctx, ctx->mx_seq, n_seq * 16))) return rc;
        if ((rc = ensure(ctx, ctx->mx_words, words.size() * 4))) return rc;
        HIP_TRY(hipMemcpyAsync(ctx->mx_seq.p, seq.data(), n_seq * 16, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ctx->mx_words.p, words.data(), words.size() * 4, hipMemcpyHostToDevice, st));
        P.mx_seq = static_cast<const uint4 *>(ctx->mx_seq.p), P.mx_words = static_cast<const uint32_t *>(ctx->mx_words.p);
        P.mx_tbase = same ? 0u : n_q;
        P.max_score = max_score, P.dx = dx, P.doe = doe, P.de = de, P.census = 0u, P.wide_exact = 0u, P.work = nullptr;
        const uint32_t seq_words = (L + 15) / 16 + 1;
        P.lds_seq_words = seq_words, P.sub_lds_words = wide_row_hw(L);
        const size_t lds_g = (size_t)score_lds_words(seq_words) * 4;
        const size_t lds_w = (size_t)wide_lds_words(seq_words, L) * 4, lds_n = (size_t)wide_lds_words_narrow(seq_words) * 4;
        const int    waves = lds_w > 12 * 1024 ? 4 : 1;  // (as the full path: rings above 12 KB are shared by four waves)
        const bool   two_phase = !glob && P.adaptive != 0u;
        // ---- tiles: C targets x R queries, at most `tile` cells (columns split as well: 1 x 1e8 is 24 tiles)
        uint64_t tile = glob ? MX_TILE_GLOBAL : std::min<uint64_t>(1ull << 18, MX_CKPT_BYTES / (WIDE_CKPT_WORDS * 4ull));
        if (ctx->opt_matrix_tile_cells > 0) tile = std::min<uint64_t>((uint64_t)ctx->opt_matrix_tile_cells, 1ull << 24);
        const uint64_t C = std::min(n_t, tile), R = std::min(n_q, tile / C);
        tile = R * C;
        if (two_phase && (rc = ensure(ctx, ctx->wide_ckpt, (size_t)tile * WIDE_CKPT_WORDS * 4))) return rc;
        P.wide_ckpt = static_cast<uint32_t *>(ctx->wide_ckpt.p), P.wide_ckpt_on = two_phase ? 1u : 0u;
        if ((rc = ensure(ctx, ctx->mx_out, (size_t)tile * 16))) return rc;
        if (ctx->mx_pin_bytes < tile * 16) {
            if (ctx->mx_pin) HIP_TRY(hipHostFree(ctx->mx_pin));
            ctx->mx_pin = nullptr, ctx->mx_pin_bytes = 0;
            HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&ctx->mx_pin), tile * 16, hipHostMallocDefault));
            ctx->mx_pin_bytes = tile * 16;
        }
        for (hipEvent_t &e : ctx->mx_ev)
            if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        uint2 *const dout = static_cast<uint2 *>(ctx->mx_out.p);
        struct Tile {
            uint64_t r0, c0, rr, cc;
        };
        // tile t's results (in buffer b) into the caller's arrays; handed-back cells into fb
        const auto scatter = [&](const Tile &t, int b) {
            const uint2 *const h = ctx->mx_pin + (uint64_t)b * tile;
            for (uint64_t r = 0; r < t.rr; r++)
                for (uint64_t j = 0; j < t.cc; j++) {
                    const uint2 v = h[r * t.cc + j];
                    if (v.x >= ST_REDO_BYTES) fb.push_back((t.r0 + r) * n_t + t.c0 + j);
                    else put(t.r0 + r, t.c0 + j, v.x, v.y);
                }
        };
        HIP_TRY(hipEventRecord(ctx->ev0, st));
        Tile     prev{};
        uint64_t c = 0;
        for (uint64_t r0 = 0; r0 < n_q; r0 += R)
            for (uint64_t c0 = 0; c0 < n_t; c0 += C, c++) {
                const Tile t{r0, c0, std::min(R, n_q - r0), std::min(C, n_t - c0)};
                const int  b = (int)(c & 1u);
                if (c >= 2) HIP_TRY(hipStreamWaitEvent(st, ctx->mx_ev[2 + b], 0));  // (buffer b's previous tile has left the device)
                const uint32_t cn = (uint32_t)(t.rr * t.cc);
                P.score_out = dout + (uint64_t)b * tile, P.chunk_first = 0u, P.chunk_n = cn;
                P.mx_r0 = t.r0, P.mx_c0 = t.c0, P.mx_cols = (uint32_t)t.cc;
                if (glob) {
                    // two launches over the tile: each kernel takes its own cells and leaves the other's slots alone
                    bool some_long = false, all_long = false;
                    if (use_long) {
                        const uint64_t tb = same ? 0u : n_q;
                        const uint64_t lr = n_lng[t.r0 + t.rr] - n_lng[t.r0], lc = n_lng[tb + t.c0 + t.cc] - n_lng[tb + t.c0];
                        some_long = lr != 0 || lc != 0, all_long = lr == t.rr || lc == t.cc;
                    }
                    if (!all_long) HIP_TRY(wfa_launch_score_matrix(P, cn, lds_g, st));
                    if (some_long) {
                        KParams PL = P;
                        PL.lds_seq_words = score_long_window(ctx->opt_score_long_window);
                        HIP_TRY(wfa_launch_score_long(true, PL, cn, (size_t)score_long_lds_words(PL.lds_seq_words) * 4, st));
                        if (!all_long) tm.n_launches++;
                    }
                } else {
                    HIP_TRY(wfa_launch_wide_score_matrix(shape, 0, waves, P, cn, lds_w, st));
                    if (two_phase) {
                        HIP_TRY(wfa_launch_wide_score_matrix(shape, 1, 1, P, cn, lds_n, st));
                        tm.n_launches++;
                    }
                }
                tm.n_launches++, tm.n_main_launches++;
                HIP_TRY(hipEventRecord(ctx->mx_ev[b], st));
                HIP_TRY(hipStreamWaitEvent(st_dn, ctx->mx_ev[b], 0));
                HIP_TRY(hipMemcpyAsync(ctx->mx_pin + (uint64_t)b * tile, P.score_out, (size_t)cn * 8, hipMemcpyDeviceToHost, st_dn));
                HIP_TRY(hipEventRecord(ctx->mx_ev[2 + b], st_dn));
                if (c >= 1) {  // the previous tile, while this one runs
                    HIP_TRY(hipEventSynchronize(ctx->mx_ev[2 + (b ^ 1)]));
                    scatter(prev, b ^ 1);
                }
                prev = t;
            }
        HIP_TRY(hipEventRecord(ctx->ev1, st));
        HIP_TRY(hipEventSynchronize(ctx->mx_ev[2 + (int)((c - 1) & 1u)]));
        scatter(prev, (int)((c - 1) & 1u));
        HIP_TRY(hipStreamSynchronize(st));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        tm.kernel_ms = tm.main_kernel_ms = ms;
        tm.main_kernel_kind = glob ? (long_main ? 24u : 21u) : 22u;
    }
    // ---- the full path: what the kernels handed back (bytes outside ACGT, a band or a length they cannot hold) -- or every cell, for a
    // penalty shape without an instance -- a batch of at most MX_FB_PAIRS cells at a time, only the score kept
    const uint64_t n_fb = on_kernel ? (uint64_t)fb.size() : n_q * n_t;
    {
        std::vector<uint64_t> qo, to;
        std::vector<uint32_t> ql, tl;
        for (uint64_t a = 0; a < n_fb; a += MX_FB_PAIRS) {
            const uint64_t n = std::min(MX_FB_PAIRS, n_fb - a);
            qo.resize(n), to.resize(n), ql.resize(n), tl.resize(n);
            for (uint64_t k = 0; k < n; k++) {
                const uint64_t x = on_kernel ? fb[a + k] : a + k, i = x / n_t, j = x % n_t;
                qo[k] = q_off[i], ql[k] = q_len[i], to[k] = t_off[j], tl[k] = t_len[j];
            }
            wfahip_results r;
            if ((rc = align_batch_entry(ctx, p, seq_blob, blob_bytes, qo.data(), ql.data(), to.data(), tl.data(), n, &r))) return rc;
            for (uint64_t k = 0; k < n; k++) {
                const uint64_t x = on_kernel ? fb[a + k] : a + k;
                const uint32_t st = (uint32_t)r.status[k], sc = r.score[k];
                if (st == ST_OK && max_score != 0u && sc > max_score) put(x / n_t, x % n_t, ST_OVER_MAX, 0u);
                else put(x / n_t, x % n_t, st, sc);
            }
            wfahip_results_free(&r);
            const wfahip_timing &f = ctx->timing;
            tm.kernel_ms += f.kernel_ms, tm.n_launches += f.n_launches, tm.arena_bytes = std::max(tm.arena_bytes, f.arena_bytes);
            if (!on_kernel) tm.main_kernel_ms += f.main_kernel_ms, tm.n_main_launches += f.n_main_launches, tm.main_kernel_kind = f.main_kernel_kind;
        }
    }
    tm.n_retried_pairs = (uint32_t)std::min<uint64_t>(n_fb, UINT32_MAX);
    tm.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    ctx->timing = tm;
    return WFAHIP_OK;
}

extern "C" int wfahip_score_matrix(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *seq_blob, uint64_t blob_bytes, const uint64_t *q_off,
                                   const uint32_t *q_len, uint64_t n_q, const uint64_t *t_off, const uint32_t *t_len, uint64_t n_t, uint32_t max_score,
                                   int32_t *status, uint32_t *score, uint64_t out_stride) {
    WFAHIP_GUARD(score_matrix_impl(ctx, p, seq_blob, blob_bytes, q_off, q_len, n_q, t_off, t_len, n_t, max_score, status, score, out_stride))
}

// ---- pre-packed input (a quarter of the bytes cross PCIe)
extern "C" int wfahip_align_batch_packed(wfahip_ctx *ctx, const wfahip_params *p, const uint32_t *packed, uint64_t n_words,
                                         const uint64_t *q_woff, const uint32_t *q_len, const uint64_t *t_woff,
                                         const uint32_t *t_len, uint64_t n_pairs, wfahip_results *out) {
    if (!ctx || !out || (!packed && n_words)) return WFAHIP_ERR_BAD_ARG;
    try {
        if (n_pairs && (!q_woff || !t_woff)) return WFAHIP_ERR_BAD_ARG;
        static const uint32_t no_words[4] = {0, 0, 0, 0};
        return align_batch_impl(ctx, p, nullptr, n_words * 16, q_woff, q_len, t_woff, t_len, n_pairs, out, packed ? packed : no_words);
    } catch (const std::bad_alloc &) {
        return WFAHIP_ERR_OOM;
    } catch (...) {
        return WFAHIP_ERR_INTERNAL;
    }
}

extern "C" uint64_t wfahip_packed_words(uint32_t len) { return ((uint64_t)len + 15) / 16 + 1; }  // (+1: the pad word the kernels' 16-base windows may read)

// Host-side packer: n_pairs (query, target) byte sequences -> 2-bit words, every sequence at a word boundary, in pair
// order (query then target).  Returns WFAHIP_ERR_UNSUPPORTED when a byte outside {A,C,G,T} is found (such a batch
// must use the byte entry: the reference compares raw bytes, wfa.go:408-454).  packed must hold
// sum(wfahip_packed_words(q_len[i]) + wfahip_packed_words(t_len[i])) words.
static int pack_pairs_impl(const uint8_t *seq_blob, const uint64_t *q_off, const uint32_t *q_len, const uint64_t *t_off,
                           const uint32_t *t_len, uint64_t n_pairs, int n_threads, uint32_t *packed, uint64_t *q_woff,
                           uint64_t *t_woff, uint64_t *n_words) {
    if (!q_off || !q_len || !t_off || !t_len || !packed || !q_woff || !t_woff || (!seq_blob && n_pairs)) return WFAHIP_ERR_BAD_ARG;
    uint64_t pos = 0;
    for (uint64_t i = 0; i < n_pairs; i++) {
        q_woff[i] = pos, pos += wfahip_packed_words(q_len[i] <= WFAHIP_MAX_SEQ_LEN ? q_len[i] : 0);
        t_woff[i] = pos, pos += wfahip_packed_words(t_len[i] <= WFAHIP_MAX_SEQ_LEN ? t_len[i] : 0);
    }
    if (n_words) *n_words = pos;
    std::atomic<int> bad{0};
    const auto       one = [&](const uint8_t *s, uint32_t len, uint32_t *dst) {
        if (len > WFAHIP_MAX_SEQ_LEN) len = 0;  // (rejected per pair by the alignment itself)
        if (pack_seq_fast(s, len, dst)) bad = 1;  // (eight bytes at a time: round 2's byte loop packed 2 GB in 34 ms on 32 threads)
    };
    const auto range = [&](uint64_t a, uint64_t b) {
        for (uint64_t i = a; i < b; i++) {
            one(seq_blob + q_off[i], q_len[i], packed + q_woff[i]);
            one(seq_blob + t_off[i], t_len[i], packed + t_woff[i]);
        }
    };
    if (n_threads < 1) n_threads = 1;
    if ((uint64_t)n_threads > n_pairs / 1024 + 1) n_threads = (int)(n_pairs / 1024 + 1);
    std::vector<std::thread> th;
    const uint64_t           per = (n_pairs + n_threads - 1) / n_threads;
    for (int t = 0; t < n_threads; t++) {
        const uint64_t a = std::min<uint64_t>(n_pairs, (uint64_t)t * per), b = std::min<uint64_t>(n_pairs, a + per);
        bool inl = n_threads == 1;
        if (!inl) {
            try {
                th.emplace_back(range, a, b);
            } catch (...) {
                inl = true;
            }
        }
        if (inl) range(a, b);
    }
    for (auto &t : th) t.join();
    return bad ? WFAHIP_ERR_UNSUPPORTED : WFAHIP_OK;
}

extern "C" int wfahip_pack_pairs(const uint8_t *seq_blob, const uint64_t *q_off, const uint32_t *q_len, const uint64_t *t_off,
                                 const uint32_t *t_len, uint64_t n_pairs, int n_threads, uint32_t *packed, uint64_t *q_woff,
                                 uint64_t *t_woff, uint64_t *n_words) {
    WFAHIP_GUARD(pack_pairs_impl(seq_blob, q_off, q_len, t_off, t_len, n_pairs, n_threads, packed, q_woff, t_woff, n_words))
}

// ---- Align (wfa.go:196) for ONE pair without the batch plumbing.
// A caller that cannot batch pays per call, not per base: through wfahip_align_batch a 1 kbp pair took 0.45-0.75 ms, of
// which the kernels were a fifth -- five launches, a dozen staged copies, thirteen result arrays.  Here the pair is
// written into a page-locked block that is mapped into the GPU's address space; the forward kernel reads the two
// sequences from there (2 KB over PCIe, inside its refill), the backtrace kernel writes the record and the CIGAR ops
// back into it, and the host waits for the stream once: one memset of the control words, two launches, no copy.
// Taken by global alignments with penalties shaped 2 : 4 : 1 (4/6/2, the default) whose sequences fit the blocked
// kernel's LDS budget and whose worst-case CIGAR fits the block; everything else -- and a pair the blocked kernel hands
// on (band wider than 64 diagonals, a byte outside ACGT, arena rows) -- goes through wfahip_align_batch: same results.
namespace {
constexpr size_t ONE_PIN_BYTES = 1u << 20, ONE_IMG_MAX = 64u << 10, ONE_REC_OFF = ONE_IMG_MAX, ONE_OPS_OFF = ONE_IMG_MAX + 256;
}

static int align_pair_impl(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *q, uint32_t n, const uint8_t *t, uint32_t m,
                           uint32_t *rec_out, uint64_t *ops_out, uint64_t ops_cap, uint64_t *n_ops) {
    if (!ctx || !p || !rec_out || !n_ops || (!ops_out && ops_cap)) return WFAHIP_ERR_BAD_ARG;
    int rc = check_params(p);
    if (rc != WFAHIP_OK) return rc;
    std::memset(rec_out, 0, REC_WORDS * 4);
    *n_ops = 0;
    if (n == 0 || m == 0) {
        rec_out[REC_STATUS] = ST_EMPTY;  // wfa.go:204-206
        return WFAHIP_OK;
    }
    if (n > WFAHIP_MAX_SEQ_LEN || m > WFAHIP_MAX_SEQ_LEN) {
        rec_out[REC_STATUS] = ST_TOO_LONG;  // wfa.go:207-209
        return WFAHIP_OK;
    }
    if (!q || !t) return WFAHIP_ERR_BAD_ARG;
    const uint32_t max_len = std::max(n, m), min_len = std::min(n, m);
    const uint32_t g = gcd_u32(gcd_u32(p->mismatch, p->gap_open + p->gap_ext), p->gap_ext ? p->gap_ext : p->mismatch);
    const uint32_t seq_words = (max_len + 15) / 16 + 1;
    const uint64_t q_cap = ((uint64_t)n + 15) & ~15ull, img = q_cap + (((uint64_t)m + 15) & ~15ull) + 64;
    // worst-case score of a global alignment under the reference's rules (first cell consumed as (mis)match):
    // every shared base a mismatch, the overhang one gap, plus one more gap for the first-cell quirk
    const uint64_t worst = (uint64_t)p->mismatch * min_len + 2ull * (p->gap_open + p->gap_ext) + (uint64_t)p->gap_ext * (max_len - min_len + 2);
    const uint32_t min_xe = std::min(p->mismatch, p->gap_ext ? p->gap_ext : p->mismatch);
    const uint64_t ops_bound = 2 * (worst / std::max(1u, min_xe)) + 64;
    // (the lone-pair instance exists for every penalty shape of wfa_fwd.hpp; round 3's paths, pair_fast = 2 / 3, for the default one)
    const int  shape = p->gap_ext != 0 ? fwd_shape(p->mismatch / g, (p->gap_open + p->gap_ext) / g, p->gap_ext / g) : -1;
    const bool fast = ctx->opt_pair_fast != 0 && ctx->opt_packed != 0 && ctx->opt_blk == 16 && ctx->force_mode < 0 && p->global_alignment &&
                      shape >= 0 && (shape == 0 || ctx->opt_pair_fast == 1) &&
                      (size_t)seq_words * 2 * 4 * (ctx->opt_pair_fast == 1 ? 1 : 4) + 16 <= (ctx->opt_pair_fast == 1 ? 64 : 20) * 1024 && img <= ONE_IMG_MAX &&
                      ONE_OPS_OFF + ops_bound * 8 <= ONE_PIN_BYTES;
    if (fast) {
        HIP_TRY(hipSetDevice(ctx->device));
        if (ctx->bt_pending) {
            (void)hipStreamSynchronize(ctx->stream2);
            ctx->bt_pending = false;
        }
        if (!ctx->one_pin) {
            HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&ctx->one_pin), ONE_PIN_BYTES, hipHostMallocMapped));
            HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&ctx->one_dev), ctx->one_pin, 0));
        }
        hipStream_t st = ctx->stream;
        // arena: rows for the worst-case score (64 words per score index), capped: what does not fit retries the usual way
        const uint64_t words = std::min<uint64_t>(((worst / g + 16) * 64 + 511) & ~511ull, std::max<uint64_t>(2048, (32ull * max_len + 511) & ~511ull));
        if ((rc = ensure(ctx, ctx->one_ctl, 1024))) return rc;
        if ((rc = ensure(ctx, ctx->redo, 64))) return rc;
        if ((rc = ensure(ctx, ctx->meta, 64))) return rc;
        if (ctx->arena.bytes < words * 4 && (rc = ensure(ctx, ctx->arena, words * 4))) return rc;
        char *const h = ctx->one_pin;
        std::memcpy(h, q, n);
        std::memcpy(h + q_cap, t, m);
        uint64_t *const offs = reinterpret_cast<uint64_t *>(h + img - 64);  // {q_off, t_off} {q_len, t_len}
        offs[0] = 0, offs[1] = q_cap;
        uint32_t *const lens = reinterpret_cast<uint32_t *>(offs + 2);
        lens[0] = n, lens[1] = m;
        uint32_t *const hrec = reinterpret_cast<uint32_t *>(h + ONE_REC_OFF);
        hrec[REC_STATUS] = ST_PENDING;
        uint32_t *const d_ctrl = static_cast<uint32_t *>(ctx->one_ctl.p);
        KParams P{};
        char *const d = ctx->one_dev;
        P.blob = reinterpret_cast<const uint8_t *>(d), P.blob_bytes = img - 64;
        P.q_off = reinterpret_cast<const uint64_t *>(d + img - 64), P.t_off = P.q_off + 1;
        P.q_len = reinterpret_cast<const uint32_t *>(d + img - 48), P.t_len = P.q_len + 1;
        P.queue_head = d_ctrl + 0, P.redo_count = d_ctrl + 1, P.ops_cursor = reinterpret_cast<unsigned long long *>(d_ctrl + 2);
        P.redo_list = static_cast<uint32_t *>(ctx->redo.p);
        P.x = p->mismatch, P.o = p->gap_open, P.e = p->gap_ext, P.oe = p->gap_open + p->gap_ext, P.g = g;
        P.global_alignment = 1, P.adaptive = p->adaptive ? 1 : 0, P.min_wf_len = p->min_wf_len, P.max_dist_diff = p->max_dist_diff;
        P.rec = reinterpret_cast<uint32_t *>(d + ONE_REC_OFF);
        P.ops = reinterpret_cast<uint64_t *>(d + ONE_OPS_OFF), P.ops_cap = (ONE_PIN_BYTES - ONE_OPS_OFF) / 8;
        P.arena = static_cast<uint32_t *>(ctx->arena.p), P.arena_words = words, P.compact_fmt = WFA_BLK_TILED ? 3u : 1u;
        P.pair_meta = static_cast<uint4 *>(ctx->meta.p);
        P.dx = P.x / g, P.doe = P.oe / g, P.de = 1, P.dm = std::max(P.dx, P.doe) + 1, P.di = 2, P.min_xe = min_xe;
        P.lds_seq_words = seq_words, P.chunk_first = 0, P.chunk_n = 1, P.n_work = 1;
        // Round 4, the lone-pair instance with the arena rows in LDS first (pair_lds): rows behind the sequences, as many as the
        // worst-case score needs or 160 KB hold; a pair that runs out of them (ST_REDO_ARENA in its record) is run again by the
        // global-memory instance, and the next calls start there (one_lds_skip).
        const uint32_t lds_off   = ((uint32_t)seq_words * 2u + 4u + 31u) & ~31u;  // words; tiles want their 128-byte lines
        const uint64_t lds_rows  = std::min<uint64_t>((worst / g + 16 + 7) & ~7ull, ((160u * 1024u - lds_off * 4u) / 256u) & ~7u);
        bool           use_lds   = ctx->opt_pair_fast == 1 && ctx->opt_pair_lds != 0 && ctx->one_lds_skip == 0 && lds_rows >= 64;
        if (ctx->one_lds_skip) ctx->one_lds_skip--;
        uint32_t launches = 0;
        for (;;) {
            hrec[REC_STATUS] = ST_PENDING;
            // (the lone-pair instance leaves its control words zeroed: only the first call, or one after another path, clears them)
            if (!(ctx->opt_pair_fast == 1 && ctx->one_ctl_clean)) HIP_TRY(hipMemsetAsync(d_ctrl, 0, 1024, st));
            ctx->one_ctl_clean = false;
            if (ctx->opt_pair_fast == 2) {  // forward kernel, then the backtrace kernel (kept for comparison: 305 us per 1 kbp pair)
                HIP_TRY(wfa_launch_fwd(0, 3, 0u, P, 1u, (size_t)seq_words * 2 * 4 * 4 + 16, st));
                HIP_TRY(wfa_launch_backtrace_one(P, st));
                launches += 2;
            } else if (ctx->opt_pair_fast == 1) {
                // ONE launch of the lone-pair instance: the whole wave on the pair, a lane per diagonal (a quarter of the
                // instructions of a step of the four-pairs-per-wave kernel -- a lone wave's step is the latency of its own instruction
                // stream), and the same wave walks the backtrace when the forward pass is done -- from the rows in LDS, or from an
                // LDS region of the global arena.
                P.fuse_bt = 1;
                if (use_lds) {
                    KParams PL = P;
                    PL.arena_words = lds_rows * 64, PL.lds_arena_off = lds_off, PL.one_n = n, PL.one_m = m;
                    HIP_TRY(wfa_launch_pair(shape, true, PL, (size_t)lds_off * 4 + (size_t)lds_rows * 256, st));
                } else {
                    HIP_TRY(wfa_launch_pair(shape, false, P, std::max<size_t>((size_t)seq_words * 2 * 4 + 16, (size_t)CompactViewWave::WORDS * 4 + 16), st));
                }
                launches++;
            } else {
                // ONE launch: the streaming instance of the forward kernel -- the wave pushes its finished pair to the done
                // queue and, once the pair queue is empty, walks it itself (stream_backtrace at the end of the kernel): one
                // launch and its gap less than forward kernel + backtrace kernel (298 against 304 us for a 1 kbp pair).  The walk
                // itself is 66-77 us either way: one lane, ~250 instructions per CIGAR op -- not its reads (walking a copy of the
                // rows in LDS took as long).
                P.done_ctl = d_ctrl + 64, P.done_q = reinterpret_cast<uint4 *>(d_ctrl + 128), P.n_stream_wgs = 0;
                P.stream_wait = 2000000;  // 20 ms of the 100 MHz clock
                HIP_TRY(wfa_launch_fwd(0, 3, (uint32_t)FWD_STREAM, P, 1u, (size_t)seq_words * 2 * 4 * 4 + 16, st));
                launches++;
            }
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(st));
            ctx->one_ctl_clean = ctx->opt_pair_fast == 1;
            if (use_lds && hrec[REC_STATUS] == ST_REDO_ARENA) {  // more rows than LDS holds: the global-memory instance
                use_lds = false, ctx->one_lds_skip = 64;
                continue;
            }
            break;
        }
        ctx->timing = wfahip_timing{};
        ctx->timing.n_launches = launches, ctx->timing.main_kernel_kind = ctx->opt_pair_fast == 1 ? 16 : 3;  // (the batch entry never makes fewer than two launches)
        if (hrec[REC_STATUS] == ST_OK) {
            const uint64_t off = (uint64_t)hrec[REC_OPS_OFF_LO] | ((uint64_t)hrec[REC_OPS_OFF_HI] << 32);
            const uint32_t len = hrec[REC_OPS_LEN];
            if (off + len <= P.ops_cap) {
                *n_ops = len;
                if (len > ops_cap) return WFAHIP_ERR_OOM;  // (*n_ops says how many the caller's buffer must hold)
                std::memcpy(rec_out, hrec, REC_WORDS * 4);
                rec_out[REC_OPS_OFF_LO] = rec_out[REC_OPS_OFF_HI] = 0;
                std::memcpy(ops_out, reinterpret_cast<const uint64_t *>(h + ONE_OPS_OFF) + off, (size_t)len * 8);
                return WFAHIP_OK;
            }
        }
        // handed on (band / bytes / arena rows): the batch entry finishes it
    }
    const uint64_t qo = 0, to = ((uint64_t)n + 15) & ~15ull;
    std::vector<uint8_t> blob(to + m);
    std::memcpy(blob.data(), q, n);
    std::memcpy(blob.data() + to, t, m);
    wfahip_results res;
    rc = wfahip_align_batch(ctx, p, blob.data(), blob.size(), &qo, &n, &to, &m, 1, &res);
    if (rc != WFAHIP_OK) return rc;
    rec_out[REC_STATUS] = (uint32_t)res.status[0];
    if (res.status[0] == WFAHIP_PAIR_OK) {
        rec_out[REC_SCORE] = res.score[0], rec_out[REC_TBEGIN] = (uint32_t)res.tbegin[0], rec_out[REC_TEND] = (uint32_t)res.tend[0];
        rec_out[REC_QBEGIN] = (uint32_t)res.qbegin[0], rec_out[REC_QEND] = (uint32_t)res.qend[0];
        rec_out[REC_ALIGN_LEN] = res.align_len[0], rec_out[REC_MATCHES] = res.matches[0], rec_out[REC_GAPS] = res.gaps[0];
        rec_out[REC_GAP_REGIONS] = res.gap_regions[0], rec_out[REC_OPS_LEN] = res.ops_len[0];
        *n_ops = res.ops_len[0];
        if (res.ops_len[0] > ops_cap) rc = WFAHIP_ERR_OOM;
        else std::memcpy(ops_out, res.ops + res.ops_off[0], (size_t)res.ops_len[0] * 8);
    }
    wfahip_results_free(&res);
    return rc;
}

extern "C" int wfahip_align_pair(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *q, uint32_t n, const uint8_t *t, uint32_t m,
                                 uint32_t *rec, uint64_t *ops, uint64_t ops_cap, uint64_t *n_ops) {
    WFAHIP_GUARD(align_pair_impl(ctx, p, q, n, t, m, rec, ops, ops_cap, n_ops))
}

// ---- one pair at a time behind the batch: submit copies the pair, collect aligns everything submitted so far
static int submit_impl(wfahip_ctx *ctx, const uint8_t *q, uint32_t n, const uint8_t *t, uint32_t m, uint64_t *ticket) {
    if (!ctx || (!q && n) || (!t && m)) return WFAHIP_ERR_BAD_ARG;
    const uint64_t pos  = ctx->sub_blob.size();
    const uint64_t qcap = ((uint64_t)std::min<uint32_t>(n, WFAHIP_MAX_SEQ_LEN + 1u) + 15) & ~15ull;
    const uint64_t tcap = ((uint64_t)std::min<uint32_t>(m, WFAHIP_MAX_SEQ_LEN + 1u) + 15) & ~15ull;
    const bool     keep = n <= WFAHIP_MAX_SEQ_LEN && m <= WFAHIP_MAX_SEQ_LEN;  // (too long: rejected per pair, nothing to copy)
    ctx->sub_blob.resize(pos + (keep ? qcap + tcap : 0));
    if (keep && n) std::memcpy(ctx->sub_blob.data() + pos, q, n);
    if (keep && m) std::memcpy(ctx->sub_blob.data() + pos + qcap, t, m);
    if (ticket) *ticket = ctx->sub_qlen.size();
    ctx->sub_qoff.push_back(pos), ctx->sub_toff.push_back(pos + qcap);
    ctx->sub_qlen.push_back(n), ctx->sub_tlen.push_back(m);
    return WFAHIP_OK;
}

extern "C" int wfahip_submit(wfahip_ctx *ctx, const uint8_t *q, uint32_t n, const uint8_t *t, uint32_t m, uint64_t *ticket) {
    WFAHIP_GUARD(submit_impl(ctx, q, n, t, m, ticket))
}

extern "C" uint64_t wfahip_pending(const wfahip_ctx *ctx) { return ctx ? ctx->sub_qlen.size() : 0; }

static int collect_impl(wfahip_ctx *ctx, const wfahip_params *p, wfahip_results *out) {
    if (!ctx || !out) return WFAHIP_ERR_BAD_ARG;
    const uint64_t n  = ctx->sub_qlen.size();
    const int      rc = align_batch_impl(ctx, p, ctx->sub_blob.data(), ctx->sub_blob.size(), ctx->sub_qoff.data(), ctx->sub_qlen.data(),
                                         ctx->sub_toff.data(), ctx->sub_tlen.data(), n, out);
    if (rc == WFAHIP_OK) {  // (on failure the submissions stay: the caller may collect again, e.g. with other parameters)
        ctx->sub_blob.clear(), ctx->sub_qoff.clear(), ctx->sub_toff.clear(), ctx->sub_qlen.clear(), ctx->sub_tlen.clear();
    }
    return rc;
}

extern "C" int wfahip_collect(wfahip_ctx *ctx, const wfahip_params *p, wfahip_results *out) { WFAHIP_GUARD(collect_impl(ctx, p, out)) }

