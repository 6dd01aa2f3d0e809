// wfa_score_entry.hip -- the score-only entries of the C-ABI (include/wfa_hip.h): wfahip_score_batch (host arrays),
// wfahip_score_batch_packed (host arrays over caller-packed 2-bit words), wfahip_score_batch_device (device-resident input),
// wfahip_score_batch_packed_device (device-resident words, with flags; wfahip_select_pairs_device compacts its survivors) and
// wfahip_score_matrix (every query against every target); wfahip_score_batch_packed_rc and wfahip_score_matrix_rc, which are the packed and
// the matrix entry with a reverse-complement flag per pair / per query row (wfa_rc.hpp), and wfahip_revcomp_packed.  The forward pass
// without arena or backtrace: wfa_score_kernel for global pairs, wfa_score_long_kernel for global reads beyond its length, the score
// instances of wfa_wide_kernel for semi-global ones (all launched by wfa_score.hip); whatever they hand back goes through the
// full path of wfahip_align_batch (wfa_entry.hip).  One router per entry over what they share: the route a call's penalties
// take, the launch geometry of a chunk or tile, its launch, and the full-path fallback.  No kernel is defined here.
#define WFA_NO_AUX_KERNELS 1  // (device functions and constants of the kernels' headers only)
#include <map>
#include "wfa_ctx.hpp"
#include "wfa_hostpack.hpp"
#include "wfa_fwd.hpp"
#include "wfa_wide.hpp"
#include "wfa_score.hpp"
#include "wfa_score_long.hpp"
#include "wfa_score_dev.hpp"
#include "wfa_matrix.hpp"

using namespace wfa;

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
    const unsigned       nt = (unsigned)std::min<uint64_t>(std::min<uint64_t>(host_pack_threads(16, true), pl.n_words / 65536 + 1), std::max<uint64_t>(n, 1));
    parallel_ranges(0, n, nt, [&](uint64_t a, uint64_t b) {
        for (uint64_t j = a; j < b; j++) {
            const uint64_t i = pl.ids[j];
            bool           bd = pack_seq_fast(seq_blob + q_off[i], q_len[i], words + pl.qw[j]);
            bd |= pack_seq_fast(seq_blob + t_off[i], t_len[i], words + pl.tw[j]);
            bad[j] = bd ? 1 : 0;
        }
    });
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

// ---- what the four routers share
namespace {
constexpr uint64_t SD_FB_PAIRS    = 1ull << 20;  // wfahip_score_batch_device, pairs per call of the full path: 64 MB of records
constexpr uint64_t MX_TILE_GLOBAL = 1ull << 22;  // wfahip_score_matrix, cells per tile of wfa_score_kernel<true>: 32 MB of {status, score}
constexpr uint64_t MX_CKPT_BYTES  = 1ull << 30;  // ... the wide kernel's checkpoints of one tile (WIDE_CKPT_WORDS words per cell in flight)
constexpr uint64_t MX_FB_PAIRS    = 1ull << 16;  // ... cells per call of the full path

// The route of a call, from its penalties: global pairs on wfa_score_kernel, semi-global ones on the wide kernel's instance of
// `shape`; on_kernel false: no instance for these penalties, every pair takes the full path.
struct ScoreRoute {
    bool glob;
    int  shape;
    bool on_kernel;
};
// ... and the penalties themselves into P, with the constants of a score-only launch
ScoreRoute score_route(KParams &P, const wfahip_params *p) {
    set_penalties(P, p);
    P.dx = P.x / P.g, P.doe = P.oe / P.g, P.de = P.e / P.g, P.census = 0u, P.wide_exact = 0u, P.work = nullptr;
    ScoreRoute R;
    R.glob      = P.global_alignment != 0u;
    R.shape     = fwd_shape(P.dx, P.doe, P.de);
    R.on_kernel = R.glob ? score_shape_ok(P.dx, P.doe, P.de) : R.shape >= 0;
    return R;
}

// Launch geometry of the chunks or tiles of a call on wfa_score_kernel / the wide kernel: the longest read they take is L bases,
// at most `in_flight` pairs run at a time (the wide kernel's checkpoints under wf-adaptive take WIDE_CKPT_WORDS words for each)
struct ScoreGeom {
    size_t lds_g, lds_w, lds_n;  // bytes of LDS: wfa_score_kernel, the wide kernel's phase 0, its phase 1
    int    waves;                // waves per pair of phase 0
    bool   two_phase;
};
int score_geometry(wfahip_ctx *ctx, KParams &P, uint32_t L, uint64_t in_flight, ScoreGeom &G) {
    const uint32_t seq_words = (L + 15) / 16 + 1;
    P.lds_seq_words = seq_words, P.sub_lds_words = wide_row_hw(L);
    G.lds_g = (size_t)score_lds_words(seq_words) * 4;
    G.lds_w = (size_t)wide_lds_words(seq_words, L) * 4, G.lds_n = (size_t)wide_lds_words_narrow(seq_words) * 4;
    G.waves = G.lds_w > 12 * 1024 ? 4 : 1;  // (as the full path: rings above 12 KB are shared by four waves)
    G.two_phase = P.global_alignment == 0u && P.adaptive != 0u;
    int rc;
    if (G.two_phase && (rc = ensure(ctx, ctx->wide_ckpt, (size_t)in_flight * WIDE_CKPT_WORDS * 4))) return rc;
    P.wide_ckpt = static_cast<uint32_t *>(ctx->wide_ckpt.p), P.wide_ckpt_on = G.two_phase ? 1u : 0u;
    return WFAHIP_OK;
}
// ... and the launch of one of them, the P.chunk_n pairs P names: wfa_score_kernel, or the wide kernel's phase 0 and, under
// wf-adaptive, its phase 1 (stage: the instances that take the pairs as P names them -- STAGE_BYTES, STAGE_MATRIX for the cells of a
// tile, STAGE_PACKED for a list over caller-packed words)
int score_launch_short(wfahip_ctx *ctx, int stage, const ScoreRoute &R, const ScoreGeom &G, const KParams &P, hipStream_t st, wfahip_timing &tm) {
    if (R.glob) {
        HIP_TRY(wfa_launch_score(stage, P, P.chunk_n, G.lds_g, st));
    } else {
        HIP_TRY(wfa_launch_wide_score(stage, R.shape, 0, G.waves, P, P.chunk_n, G.lds_w, st));
        if (G.two_phase) {
            HIP_TRY(wfa_launch_wide_score(stage, R.shape, 1, 1, P, P.chunk_n, G.lds_n, st));
            tm.n_launches++;
        }
    }
    tm.n_launches++, tm.n_main_launches++;
    return WFAHIP_OK;
}

// The full path's call and its bookkeeping, shared by the byte and the packed fallback: align(&r) aligns the n pairs the caller laid
// out (under the call's bound), put(k, status, score) takes pair k's result, and the inner call's timing is folded into tm.
template <class Align, class Put>
int score_fallback_run(wfahip_ctx *ctx, uint64_t n, uint32_t max_score, bool on_kernel, wfahip_timing &tm, const Align &align, const Put &put) {
    wfahip_results r;
    int            rc;
    {
        BoundScope bound(ctx, max_score);  // (the full path stops and filters by it: wfahip_align_batch_bounded's path)
        rc = align(&r);
    }
    if (rc) return rc;
    for (uint64_t k = 0; k < n; k++) put(k, (uint32_t)r.status[k], r.score[k]);
    wfahip_results_free(&r);
    const wfahip_timing &f = ctx->timing;
    tm.kernel_ms += f.kernel_ms, tm.n_launches += f.n_launches, tm.arena_bytes = std::max(tm.arena_bytes, f.arena_bytes);
    if (!on_kernel) tm.main_kernel_ms += f.main_kernel_ms, tm.n_main_launches += f.n_main_launches, tm.main_kernel_kind = f.main_kernel_kind;
    return WFAHIP_OK;
}
// The full path for n pairs the kernels handed back (bytes outside ACGT, a band or a length they cannot hold, a shape without an
// instance), only the score kept: pair k is query pick(k).first against target pick(k).second of the caller's arrays, and its
// result goes to put(k, status, score) -- ST_OVER_MAX beyond max_score, as the kernels say it.  The timing of the inner call is
// folded into tm; it is the call's main kernel when no score kernel ran (!on_kernel).
template <class Pick, class Put>
int score_fallback(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *seq_blob, uint64_t blob_bytes, const uint64_t *q_off,
                   const uint32_t *q_len, const uint64_t *t_off, const uint32_t *t_len, uint64_t n, uint32_t max_score, bool on_kernel,
                   wfahip_timing &tm, const Pick &pick, const Put &put) {
    std::vector<uint64_t> qo(n), to(n);
    std::vector<uint32_t> ql(n), tl(n);
    for (uint64_t k = 0; k < n; k++) {
        const std::pair<uint64_t, uint64_t> s = pick(k);
        qo[k] = q_off[s.first], ql[k] = q_len[s.first], to[k] = t_off[s.second], tl[k] = t_len[s.second];
    }
    return score_fallback_run(
        ctx, n, max_score, on_kernel, tm,
        [&](wfahip_results *r) { return align_batch_entry(ctx, p, seq_blob, blob_bytes, qo.data(), ql.data(), to.data(), tl.data(), n, r); }, put);
}
}  // namespace

// The launch section of a score batch, shared by wfahip_score_batch, wfahip_score_batch_packed and wfahip_score_batch_device: P names
// the batch (device pointers; stage says whether its offsets count bytes of P.blob or words of P.mx_words), score_out, the
// penalties and max_score.  LDS sizing from max_len, chunks of 2^24 (global) / 2^18 (semi-global: the wide
// kernel's checkpoints take WIDE_CKPT_WORDS words per pair of a chunk) pairs, the wide kernel's two phases under wf-adaptive, and
// the n_listed pairs of ctx->mx_seq / mx_words on wfa_score_long_kernel behind the short launch.  Records ctx->ev0 before the
// first launch and ctx->ev1 behind the last; synchronises nothing.  n_long: the long pairs of the batch (listed or not).
// n_rc_jobs: the listed pairs whose query is flagged -- wfa_rc_words_kernel writes the words their entries name (ctx->rc_jobs) first.
static int score_launch(wfahip_ctx *ctx, int stage, KParams &P, const ScoreRoute &R, uint64_t n_pairs, uint32_t max_len, bool skip_short, uint64_t n_listed,
                        uint64_t n_long, hipStream_t st, wfahip_timing &tm, bool &long_main, uint64_t n_rc_jobs = 0) {
    int            rc;
    const uint32_t L     = std::min<uint32_t>(max_len, R.glob ? SCORE_MAX_LEN : WIDE_MAX_LEN);  // (longer pairs come back ST_REDO_LDS)
    const uint64_t chunk = R.glob ? (1ull << 24) : (1ull << 18);
    ScoreGeom      G;
    if ((rc = score_geometry(ctx, P, L, std::min<uint64_t>(chunk, n_pairs), G))) return rc;
    if (!ctx->ev0) HIP_TRY(hipEventCreate(&ctx->ev0));
    if (!ctx->ev1) HIP_TRY(hipEventCreate(&ctx->ev1));
    HIP_TRY(hipEventRecord(ctx->ev0, st));
    if (n_rc_jobs) {
        HIP_TRY(wfa_launch_rc_words(static_cast<const uint4 *>(ctx->rc_jobs.p), static_cast<uint32_t *>(ctx->mx_words.p), (uint32_t)n_rc_jobs, st));
        tm.n_launches++;
    }
    for (uint64_t c0 = 0; c0 < n_pairs && !skip_short; c0 += chunk) {
        P.chunk_first = (uint32_t)c0, P.chunk_n = (uint32_t)std::min<uint64_t>(chunk, n_pairs - c0);
        if ((rc = score_launch_short(ctx, stage, R, G, P, st, tm))) return rc;
    }
    // the listed long pairs, behind wfa_score_kernel on the same stream: their slots (ST_REDO_LDS there) take the long kernel's result
    long_main = n_listed > n_pairs - n_long;  // it took more pairs of the call than the short kernel
    if (n_listed) {
        KParams PL = P;
        // (the words the table points into: ctx->mx_words, where the byte entries packed them and the host packed entry uploaded them --
        // or, the call naming words that are not the context's, wfahip_score_batch_packed_device's: the caller's own)
        if (stage != STAGE_PACKED) PL.mx_words = static_cast<const uint32_t *>(ctx->mx_words.p);
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

// ---- score only (wfahip_score_batch): host arrays in, host arrays out
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
    KParams            P{};
    const ScoreRoute   R = score_route(P, p);
    // ---- global pairs beyond wfa_score_kernel's length: wfa_score_long_kernel takes them when the call holds at least "score_long_min"
    // of them; they are packed here (host threads) into the context's page-locked word buffer and listed
    ScoreLongPlan         lp;
    std::vector<uint4>    ltab;    // two entries per listed pair
    std::vector<uint64_t> lbytes;  // long pairs with a byte outside ACGT: the full path
    bool                  use_long = false;
    if (R.on_kernel && R.glob && n_pairs <= UINT32_MAX) {
        score_long_plan(q_len, t_len, n_pairs, lp);
        use_long = !lp.ids.empty() && (int64_t)lp.ids.size() >= ctx->opt_score_long_min;
    }
    // (no page-locked memory for the words: these pairs take the full path, as below the gate)
    const size_t need = (size_t)(lp.n_words + 4) * 4;
    if (use_long && grow_pinned(ctx->pack_pin, ctx->pack_pin_bytes, need, need / 8) != hipSuccess) use_long = false;
    if (use_long) score_long_pack(seq_blob, q_off, q_len, t_off, t_len, lp, ctx->pack_pin, ltab, lbytes);
    const uint64_t n_listed   = ltab.size() / 2;
    const bool     skip_short = use_long && lp.ids.size() == n_pairs;  // every pair is long: nothing for wfa_score_kernel
    if (R.on_kernel) {
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
        bool long_main = false;
        if ((rc = score_launch(ctx, STAGE_BYTES, P, R, n_pairs, max_len, skip_short, n_listed, lp.ids.size(), st, tm, long_main))) return rc;
        HIP_TRY(hipMemcpyAsync(res.data(), ctx->score_out.p, n_pairs * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        tm.kernel_ms = tm.main_kernel_ms = ms;
        tm.main_kernel_kind = R.glob ? (long_main ? K_SCORE_LONG : K_SCORE) : K_SCORE_WIDE;
        // (long pairs that were not listed: wfa_score_kernel said ST_REDO_LDS, or never saw them)
        for (const uint64_t i : lbytes) res[i] = make_uint2(ST_REDO_BYTES, 0u);
    } else {
        for (uint64_t i = 0; i < n_pairs; i++) res[i] = make_uint2(ST_REDO_BAND, 0u);
    }
    std::vector<uint64_t> fb;  // what the kernels handed back
    for (uint64_t i = 0; i < n_pairs; i++)
        if (res[i].x >= ST_REDO_BYTES) fb.push_back(i);
    if (!fb.empty() && (rc = score_fallback(ctx, p, seq_blob, blob_bytes, q_off, q_len, t_off, t_len, fb.size(), max_score, R.on_kernel, tm,
                                            [&](uint64_t k) { return std::make_pair(fb[k], fb[k]); },
                                            [&](uint64_t k, uint32_t st, uint32_t sc) { res[fb[k]] = make_uint2(st, sc); })))
        return rc;
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

// ---- score only on caller-packed input (wfahip_score_batch_packed): score_batch_impl over the words of wfahip_pack_pairs.  The n_words
// words go up once, into ctx->mx_words, and the four arrays behind them; the packed pair-list instances of the score kernels copy a
// pair's words into LDS from there (q_woff / t_woff are their P.q_off / P.t_off), and wfa_score_long_kernel's table points INTO the
// same words -- eight words per long pair built here, no sequence packed or uploaded a second time.  What the kernels hand back is
// gathered, those pairs' words only, into a buffer of this entry's own and aligned through the packed full path.
// wfahip_score_batch_packed_rc is the same entry with a flag per pair: a flagged pair scores the REVERSE COMPLEMENT of its query.  The
// kernels make its words as they stage them (mx_stage, wfa_rc.hpp) -- nothing is stored or sent twice; the flagged long queries are
// written once behind the uploaded words (wfa_rc_words_kernel) and the long table names them there; the gather below makes the words of the
// flagged pairs the kernels hand back with the same rc_word.
namespace {
// words of one sequence as wfahip_pack_pairs writes them: the bits of the last word beyond the last base and the pad word zero
void copy_packed_seq(const uint32_t *src, uint32_t len, uint32_t *dst) {
    const uint32_t nw = (len + 15u) >> 4, tail = len & 15u;
    std::memcpy(dst, src, (size_t)nw * 4);
    if (tail) dst[nw - 1] &= (1u << (2u * tail)) - 1u;
    dst[nw] = 0u;
}
// ... and those of its reverse complement
void revcomp_packed_seq(const uint32_t *src, uint32_t len, uint32_t *dst) {
    const uint32_t nw = (len + 15u) >> 4;
    for (uint32_t j = 0; j < nw; j++) dst[j] = rc_word(src, len, j);
    dst[nw] = 0u;
}
}  // namespace

// Host only: the reverse complement of one packed sequence, as wfahip_pack_pairs would have written it (include/wfa_hip.h)
extern "C" int wfahip_revcomp_packed(const uint32_t *src, uint32_t len, uint32_t *dst) {
    if (!dst || (!src && len) || len > WFAHIP_MAX_SEQ_LEN) return WFAHIP_ERR_BAD_ARG;
    if (len == 0) {
        for (uint64_t j = 0; j < wfahip_packed_words(0); j++) dst[j] = 0u;
        return WFAHIP_OK;
    }
    revcomp_packed_seq(src, len, dst);
    return WFAHIP_OK;
}

static int score_batch_packed_impl(wfahip_ctx *ctx, const wfahip_params *p, const uint32_t *packed, uint64_t n_words, const uint64_t *q_woff,
                                   const uint32_t *q_len, const uint64_t *t_woff, const uint32_t *t_len, const uint8_t *q_rc, uint64_t n_pairs,
                                   uint32_t max_score, wfahip_scores *out) {
    // (every check before any device work, and none dereferences ctx)
    if (!ctx || !p || !out) return WFAHIP_ERR_BAD_ARG;
    std::memset(out, 0, sizeof *out);
    if (!packed && n_words) return WFAHIP_ERR_BAD_ARG;
    if (n_pairs && (!q_woff || !q_len || !t_woff || !t_len)) return WFAHIP_ERR_BAD_ARG;
    // every pair that is neither empty nor too long has the words of both sequences, pad words included, inside the buffer (written so
    // that a hostile 64-bit offset cannot wrap the sum around); the same pass finds the longest read and the long global pairs
    uint32_t max_len = 1;
    uint64_t n_long  = 0;
    for (uint64_t i = 0; i < n_pairs; i++) {
        if (!(q_len[i] && t_len[i] && q_len[i] <= WFAHIP_MAX_SEQ_LEN && t_len[i] <= WFAHIP_MAX_SEQ_LEN)) continue;
        const uint64_t qw = wfahip_packed_words(q_len[i]), tw = wfahip_packed_words(t_len[i]);
        if (q_woff[i] > n_words || qw > n_words - q_woff[i] || t_woff[i] > n_words || tw > n_words - t_woff[i]) return WFAHIP_ERR_BAD_ARG;
        const uint32_t ml = std::max(q_len[i], t_len[i]);
        max_len = std::max(max_len, ml);
        n_long += ml > SCORE_MAX_LEN;
    }
    int rc = check_params(p);
    if (rc) return rc;
    if (n_pairs == 0) return WFAHIP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const auto t_start = std::chrono::steady_clock::now();
    q_rc = any_flag(q_rc, n_pairs);
    std::vector<uint2> res(n_pairs);
    wfahip_timing      tm{};
    KParams            P{};
    const ScoreRoute   R = score_route(P, p);
    if (R.on_kernel) {
        // ---- global pairs beyond wfa_score_kernel's length, when the call holds at least "score_long_min" of them: listed for
        // wfa_score_long_kernel where they lie in the caller's words
        const bool         use_long = R.glob && n_pairs <= UINT32_MAX && n_long != 0 && (int64_t)n_long >= ctx->opt_score_long_min;
        std::vector<uint4> ltab;  // two entries per long pair
        // a flagged long pair's query entry names words behind the uploaded ones (from word n_words + 4 on, each query with its pad word),
        // which wfa_rc_words_kernel writes: a job per distinct {the caller's words, length} among such pairs, {those words} -- one query
        // flagged against fifty long targets is written once.  (Keyed by offset AND length: the reverse complement of a prefix is no prefix
        // of the reverse complement.)  Device memory only: a quarter of a byte per base of those queries
        std::vector<uint4>                                    jobs;
        std::map<std::pair<uint64_t, uint32_t>, uint64_t>     rc_at;
        uint64_t                                              rc_end = n_words + 4;
        if (use_long) {
            ltab.reserve(2 * n_long);
            for (uint64_t i = 0; i < n_pairs; i++) {
                if (!(q_len[i] && t_len[i] && q_len[i] <= WFAHIP_MAX_SEQ_LEN && t_len[i] <= WFAHIP_MAX_SEQ_LEN)) continue;
                if (std::max(q_len[i], t_len[i]) <= SCORE_MAX_LEN) continue;
                uint64_t qw = q_woff[i];
                if (q_rc && q_rc[i]) {
                    const auto at = rc_at.emplace(std::make_pair(qw, q_len[i]), rc_end);
                    if (at.second) {
                        jobs.push_back(make_uint4((uint32_t)qw, (uint32_t)(qw >> 32), q_len[i], 0u));
                        jobs.push_back(make_uint4((uint32_t)rc_end, (uint32_t)(rc_end >> 32), 0u, 0u));
                        rc_end += wfahip_packed_words(q_len[i]);
                    }
                    qw = at.first->second;
                }
                ltab.push_back(make_uint4((uint32_t)qw, (uint32_t)(qw >> 32), q_len[i], (uint32_t)i));
                ltab.push_back(make_uint4((uint32_t)t_woff[i], (uint32_t)(t_woff[i] >> 32), t_len[i], 0u));
            }
        }
        const uint64_t n_listed   = ltab.size() / 2;
        const bool     skip_short = use_long && n_long == n_pairs;  // every pair is long: nothing for wfa_score_kernel
        hipStream_t    st         = ctx->stream;
        if ((rc = ensure(ctx, ctx->score_out, n_pairs * 8))) return rc;
        if ((rc = ensure(ctx, ctx->mx_words, (size_t)(rc_end + 4) * 4))) return rc;  // (+16 bytes, as in_packed has)
        ctx->sd_n_words = ctx->sd_n_listed = 0;  // (what wfahip_score_batch_device left there is gone)
        if (n_words) HIP_TRY(hipMemcpyAsync(ctx->mx_words.p, packed, (size_t)n_words * 4, hipMemcpyHostToDevice, st));
        if (!skip_short) {
            if ((rc = ensure(ctx, ctx->in_qoff, n_pairs * 8))) return rc;
            if ((rc = ensure(ctx, ctx->in_toff, n_pairs * 8))) return rc;
            if ((rc = ensure(ctx, ctx->in_qlen, n_pairs * 4))) return rc;
            if ((rc = ensure(ctx, ctx->in_tlen, n_pairs * 4))) return rc;
            HIP_TRY(hipMemcpyAsync(ctx->in_qoff.p, q_woff, n_pairs * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(ctx->in_toff.p, t_woff, n_pairs * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(ctx->in_qlen.p, q_len, n_pairs * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(ctx->in_tlen.p, t_len, n_pairs * 4, hipMemcpyHostToDevice, st));
            if (q_rc) {
                if ((rc = ensure(ctx, ctx->in_rc, n_pairs))) return rc;
                HIP_TRY(hipMemcpyAsync(ctx->in_rc.p, q_rc, n_pairs, hipMemcpyHostToDevice, st));
                P.q_rc = static_cast<const uint8_t *>(ctx->in_rc.p);
            }
        }
        if (n_listed) {
            if ((rc = ensure(ctx, ctx->mx_seq, ltab.size() * 16))) return rc;
            HIP_TRY(hipMemcpyAsync(ctx->mx_seq.p, ltab.data(), ltab.size() * 16, hipMemcpyHostToDevice, st));
        }
        if (!jobs.empty()) {
            if ((rc = ensure(ctx, ctx->rc_jobs, jobs.size() * 16))) return rc;
            HIP_TRY(hipMemcpyAsync(ctx->rc_jobs.p, jobs.data(), jobs.size() * 16, hipMemcpyHostToDevice, st));
        }
        P.mx_words = static_cast<const uint32_t *>(ctx->mx_words.p);
        P.q_off = static_cast<const uint64_t *>(ctx->in_qoff.p), P.t_off = static_cast<const uint64_t *>(ctx->in_toff.p);  // (in words)
        P.q_len = static_cast<const uint32_t *>(ctx->in_qlen.p), P.t_len = static_cast<const uint32_t *>(ctx->in_tlen.p);
        P.score_out = static_cast<uint2 *>(ctx->score_out.p), P.max_score = max_score;
        bool long_main = false;
        if ((rc = score_launch(ctx, STAGE_PACKED, P, R, n_pairs, max_len, skip_short, n_listed, n_long, st, tm, long_main, jobs.size() / 2))) return rc;
        HIP_TRY(hipMemcpyAsync(res.data(), ctx->score_out.p, n_pairs * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        tm.kernel_ms = tm.main_kernel_ms = ms;
        tm.main_kernel_kind = R.glob ? (long_main ? K_SCORE_LONG : K_SCORE) : K_SCORE_WIDE;
    } else {
        for (uint64_t i = 0; i < n_pairs; i++) res[i] = make_uint2(ST_REDO_BAND, 0u);
    }
    // ---- what the kernels handed back (a band or a length they cannot hold, a shape without an instance; never ST_REDO_BYTES): those
    // pairs' words, query then target at fresh offsets, as wfahip_pack_pairs would have written them -- the full path under the bound
    std::vector<uint64_t> fb;
    for (uint64_t i = 0; i < n_pairs; i++)
        if (res[i].x >= ST_REDO_BYTES) fb.push_back(i);
    if (!fb.empty()) {
        const uint64_t        n = fb.size();
        std::vector<uint64_t> qo(n), to(n);
        std::vector<uint32_t> ql(n), tl(n);
        uint64_t              pos = 0;
        // (a shape without an instance hands back EVERY pair, the empty and the too long ones too: the full path says their status from
        // the lengths alone, and their offsets, which nothing has validated, are never looked at -- they are laid out as wfahip_pack_pairs
        // lays them out, a pad word each)
        std::vector<uint8_t> valid(n);
        for (uint64_t k = 0; k < n; k++) {
            const uint64_t i = fb[k];
            ql[k] = q_len[i], tl[k] = t_len[i];
            valid[k] = ql[k] && tl[k] && ql[k] <= WFAHIP_MAX_SEQ_LEN && tl[k] <= WFAHIP_MAX_SEQ_LEN;
            qo[k] = pos, pos += wfahip_packed_words(valid[k] ? ql[k] : 0);
            to[k] = pos, pos += wfahip_packed_words(valid[k] ? tl[k] : 0);
        }
        std::vector<uint32_t> words(pos + 4);
        parallel_ranges(0, n, (unsigned)std::min<uint64_t>(host_pack_threads(16, true), pos / 65536 + 1), [&](uint64_t a, uint64_t b) {
            for (uint64_t k = a; k < b; k++) {
                if (!valid[k]) continue;  // (the vector's zeros are its two pad words)
                (q_rc && q_rc[fb[k]] ? revcomp_packed_seq : copy_packed_seq)(packed + q_woff[fb[k]], ql[k], words.data() + qo[k]);
                copy_packed_seq(packed + t_woff[fb[k]], tl[k], words.data() + to[k]);
            }
        });
        if ((rc = score_fallback_run(
                 ctx, n, max_score, R.on_kernel, tm,
                 [&](wfahip_results *r) { return align_batch_packed_entry(ctx, p, words.data(), pos, qo.data(), ql.data(), to.data(), tl.data(), n, r); },
                 [&](uint64_t k, uint32_t st, uint32_t sc) { res[fb[k]] = make_uint2(st, sc); })))
            return rc;
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

extern "C" int wfahip_score_batch_packed(wfahip_ctx *ctx, const wfahip_params *p, const uint32_t *packed, uint64_t n_words,
                                         const uint64_t *q_woff, const uint32_t *q_len, const uint64_t *t_woff, const uint32_t *t_len,
                                         uint64_t n_pairs, uint32_t max_score, wfahip_scores *out) {
    WFAHIP_GUARD(score_batch_packed_impl(ctx, p, packed, n_words, q_woff, q_len, t_woff, t_len, nullptr, n_pairs, max_score, out))
}
extern "C" int wfahip_score_batch_packed_rc(wfahip_ctx *ctx, const wfahip_params *p, const uint32_t *packed, uint64_t n_words,
                                            const uint64_t *q_woff, const uint32_t *q_len, const uint64_t *t_woff, const uint32_t *t_len,
                                            const uint8_t *q_rc, uint64_t n_pairs, uint32_t max_score, wfahip_scores *out) {
    WFAHIP_GUARD(score_batch_packed_impl(ctx, p, packed, n_words, q_woff, q_len, t_woff, t_len, q_rc, n_pairs, max_score, out))
}

// ---- score only on device-resident input (wfahip_score_batch_device): score_batch_impl with everything it does on the host done by
// the kernels of wfa_score_dev.hpp.  The host sees three blocks of SDC_WORDS counters -- after the plan (bounds flag, longest
// length, long pairs, their words), after the list (listed pairs) when long pairs run, after the redo count (pairs of the full path,
// their bases, their longest length) -- and nothing else of the batch.
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
    KParams          P{};
    const ScoreRoute R = score_route(P, p);

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
    S.want_long = (R.on_kernel && R.glob) ? 1u : 0u;
    if ((rc = count_and_scan(SDK_PLAN_COUNT, n_pairs, SDC_N_LONG, SDC_N_WORDS))) return rc;
    if ((rc = fetch_ctl())) return rc;
    if (hc[SDC_BOUNDS] != 0) return WFAHIP_ERR_BAD_ARG;
    if (max_len == 0) max_len = (uint32_t)std::max<uint64_t>(1, hc[SDC_MAX_LEN]);
    const uint64_t n_long = hc[SDC_N_LONG], n_words = hc[SDC_N_WORDS];
    const bool     use_long = n_long != 0 && (int64_t)n_long >= ctx->opt_score_long_min;
    uint64_t       n_listed = 0;
    if (R.on_kernel && (rc = ensure(ctx, ctx->score_out, n_pairs * 8))) return rc;
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
    if (R.on_kernel) {
        const bool skip_short = use_long && n_long == n_pairs;
        P.blob = S.blob, P.blob_bytes = blob_bytes, P.q_off = S.q_off, P.t_off = S.t_off, P.q_len = S.q_len, P.t_len = S.t_len;
        P.score_out = S.score_out, P.max_score = max_score;
        bool long_main = false;
        if ((rc = score_launch(ctx, STAGE_BYTES, P, R, n_pairs, max_len, skip_short, n_listed, use_long ? n_long : 0, st, tm, long_main))) return rc;
        tm.main_kernel_kind = R.glob ? (long_main ? K_SCORE_LONG : K_SCORE) : K_SCORE_WIDE;
    }
    // ---- what they handed back (every pair, for a shape without an instance): counted, then gathered in pair order
    S.all = R.on_kernel ? 0u : 1u;
    if ((rc = count_and_scan(SDK_REDO_COUNT, n_pairs, SDC_N_REDO, SDC_REDO_SUM))) return rc;
    if (R.on_kernel && (rc = launch(SDK_FINISH, n_pairs, SD_BLOCK))) return rc;
    if ((rc = fetch_ctl())) return rc;
    if (R.on_kernel) {
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
                uint64_t   needed = 0;
                BoundScope bound(ctx, max_score);  // (the full path stops and filters by it)
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
            if (!R.on_kernel && a == 0) tm.main_kernel_ms = f.main_kernel_ms, tm.n_main_launches = f.n_main_launches, tm.main_kernel_kind = f.main_kernel_kind;
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

// ---- score only on device-resident packed input, both strands (wfahip_score_batch_packed_device): score_batch_packed_impl with
// everything it does on the host done by the kernels at the end of wfa_score_dev.hpp, a sibling of score_batch_device_impl.  The host
// sees two blocks of SDC_WORDS counters -- after the plan (bounds verdict, longest read, whether a flag is set, long pairs, the words
// of the flagged long queries' reverse complements), after the redo count (pairs of the full path, their words, their longest read).
// Packed input has no byte outside ACGT: the plan's write launch emits wfa_score_long_kernel's table itself, pointing into the caller's
// words; a flagged long query is read from ctx->mx_words, where wfa_score_rcq_kernel has written its reverse complement (the caller's
// buffer cannot be written behind).  The pairs handed back have their words gathered into ctx->sd_words, flags applied, and take
// align_packed_device_impl without flags.
static int score_batch_packed_device_impl(wfahip_ctx *ctx, const wfahip_params *p, const void *d_packed, uint64_t n_words, const void *d_q_woff,
                                          const void *d_q_len, const void *d_t_woff, const void *d_t_len, const void *d_q_rc, uint64_t n_pairs,
                                          uint32_t max_len, uint32_t max_score, void *d_status, void *d_score, hipStream_t st) {
    // (none of these checks dereferences ctx)
    if (!ctx || !p) return WFAHIP_ERR_BAD_ARG;
    if (n_pairs && (!d_q_woff || !d_q_len || !d_t_woff || !d_t_len || !d_status || !d_score)) return WFAHIP_ERR_BAD_ARG;
    if (!d_packed && n_words) return WFAHIP_ERR_BAD_ARG;
    if (n_pairs > 0xFFFFFFF0ull || n_words > (1ull << 58)) return WFAHIP_ERR_BAD_ARG;  // (align_packed_device_impl's limits)
    int rc = check_params(p);
    if (rc) return rc;
    if (n_pairs == 0) return WFAHIP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (!st) st = ctx->stream;
    const auto    t_start = std::chrono::steady_clock::now();
    wfahip_timing tm{};
    ctx->sd_n_words = ctx->sd_n_listed = 0;  // (what wfahip_score_batch_device left in mx_words / mx_seq is gone)
    KParams          P{};
    const ScoreRoute R = score_route(P, p);

    const uint64_t n_tiles = (n_pairs + SD_TILE - 1) / SD_TILE;
    if ((rc = ensure(ctx, ctx->sd_ctl, SDC_WORDS * 8))) return rc;
    if ((rc = ensure(ctx, ctx->sd_blk, n_tiles * sizeof(SDSum)))) return rc;
    SDParams S{};
    // (n_words == 0: every pair is empty or too long and no word is read -- the kernels still get an address)
    S.pk_words = d_packed ? static_cast<const uint32_t *>(d_packed) : reinterpret_cast<const uint32_t *>(ctx->sd_ctl.p);
    S.n_words = n_words, S.q_rc = static_cast<const uint8_t *>(d_q_rc);
    S.q_off = static_cast<const uint64_t *>(d_q_woff), S.t_off = static_cast<const uint64_t *>(d_t_woff);
    S.q_len = static_cast<const uint32_t *>(d_q_len), S.t_len = static_cast<const uint32_t *>(d_t_len);
    S.ctl = static_cast<unsigned long long *>(ctx->sd_ctl.p), S.blk = static_cast<SDSum *>(ctx->sd_blk.p);
    S.d_status = static_cast<int32_t *>(d_status), S.d_score = static_cast<uint32_t *>(d_score), S.max_score = max_score;
    const auto count_and_scan = [&](int k, uint64_t items, uint32_t c_cnt, uint32_t c_wt) -> int {
        const uint64_t tiles = (items + SD_TILE - 1) / SD_TILE;
        SDParams       T = S;
        T.n = items;
        HIP_TRY(wfa_launch_score_dev(k, T, (uint32_t)tiles, st));
        T.n = tiles, T.c_cnt = c_cnt, T.c_wt = c_wt;
        HIP_TRY(wfa_launch_score_dev(SDK_SCAN, T, 1, st));
        return WFAHIP_OK;
    };
    const auto launch = [&](int k, uint64_t items, uint64_t groups) -> int {
        SDParams T = S;
        T.n = items;
        HIP_TRY(wfa_launch_score_dev(k, T, (uint32_t)groups, st));
        return WFAHIP_OK;
    };
    uint64_t   hc[SDC_WORDS];
    const auto fetch_ctl = [&]() -> int {  // (through the context's pinned block: a pageable copy of 64 bytes costs 0.3 ms)
        HIP_TRY(hipMemcpyAsync(ctx->hpin + HPIN_CTRL, S.ctl, SDC_WORDS * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        std::memcpy(hc, ctx->hpin + HPIN_CTRL, SDC_WORDS * 8);
        return WFAHIP_OK;
    };

    // ---- plan: bounds in words, the longest read, whether a flag is set, the long pairs.  No kernel that reads a packed word runs
    // before its verdict is in
    HIP_TRY(hipMemsetAsync(S.ctl, 0, SDC_WORDS * 8, st));
    S.want_long = (R.on_kernel && R.glob) ? 1u : 0u;
    if ((rc = count_and_scan(SDK_PK_PLAN_COUNT, n_pairs, SDC_N_LONG, SDC_N_WORDS))) return rc;
    if ((rc = fetch_ctl())) return rc;
    if (hc[SDC_BOUNDS] != 0) return WFAHIP_ERR_BAD_ARG;
    if (max_len == 0) max_len = (uint32_t)std::max<uint64_t>(1, hc[SDC_MAX_LEN]);
    if (hc[SDC_ANY_RC] == 0) S.q_rc = nullptr;  // a call whose flags are all zero is the call without flags: the same route
    const uint64_t n_long = hc[SDC_N_LONG], rc_words = hc[SDC_N_WORDS];
    const bool     use_long = n_long != 0 && (int64_t)n_long >= ctx->opt_score_long_min;
    if (R.on_kernel) {
        if ((rc = ensure(ctx, ctx->score_out, n_pairs * 8))) return rc;
        S.score_out = static_cast<uint2 *>(ctx->score_out.p);
        if (use_long) {
            // ---- the long pairs: tabled where they lie in the caller's words; the flagged ones' queries reverse-complemented into
            // scratch, one per flagged long pair
            if ((rc = ensure(ctx, ctx->mx_seq, n_long * 32))) return rc;
            if ((rc = ensure(ctx, ctx->mx_words, (size_t)(rc_words + 4) * 4))) return rc;
            S.table = static_cast<uint4 *>(ctx->mx_seq.p), S.rc_words = static_cast<uint32_t *>(ctx->mx_words.p);
            if ((rc = launch(SDK_PK_PLAN_WRITE, n_pairs, n_tiles))) return rc;
            if (rc_words && (rc = launch(SDK_PK_RCQ, n_long, n_long))) return rc;
            if (rc_words) tm.n_launches++;
        }
        // ---- the score kernels, as wfahip_score_batch_packed launches them
        const bool skip_short = use_long && n_long == n_pairs;
        P.mx_words = S.pk_words, P.mx_rc_words = static_cast<const uint32_t *>(ctx->mx_words.p);
        P.q_off = S.q_off, P.t_off = S.t_off, P.q_len = S.q_len, P.t_len = S.t_len, P.q_rc = S.q_rc;
        P.score_out = S.score_out, P.max_score = max_score;
        bool long_main = false;
        if ((rc = score_launch(ctx, STAGE_PACKED, P, R, n_pairs, max_len, skip_short, use_long ? n_long : 0, n_long, st, tm, long_main, 0))) return rc;
        tm.main_kernel_kind = R.glob ? (long_main ? K_SCORE_LONG : K_SCORE) : K_SCORE_WIDE;
    }
    // ---- what they handed back (every pair, for a shape without an instance): counted, then gathered in pair order
    S.all = R.on_kernel ? 0u : 1u;
    if ((rc = count_and_scan(SDK_PK_REDO_COUNT, n_pairs, SDC_N_REDO, SDC_REDO_SUM))) return rc;
    if (R.on_kernel && (rc = launch(SDK_FINISH, n_pairs, (n_pairs + SD_BLOCK - 1) / SD_BLOCK))) return rc;
    if ((rc = fetch_ctl())) return rc;
    if (R.on_kernel) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        tm.kernel_ms = tm.main_kernel_ms = ms;
    }
    const uint64_t n_redo = hc[SDC_N_REDO], g_words = hc[SDC_REDO_SUM];
    const uint32_t fb_max = (uint32_t)std::max<uint64_t>(1, hc[SDC_REDO_MAX]);
    if (n_redo) {
        // r_qoff | r_toff | r_id | r_qlen | r_tlen | r_rc
        if ((rc = ensure(ctx, ctx->sd_redo, n_redo * 29))) return rc;
        if ((rc = ensure(ctx, ctx->sd_words, (size_t)(g_words + 4) * 4))) return rc;  // (+16 bytes, as the entry asks of its caller)
        S.r_qoff = static_cast<uint64_t *>(ctx->sd_redo.p), S.r_toff = S.r_qoff + n_redo;
        S.r_id = reinterpret_cast<uint32_t *>(S.r_toff + n_redo), S.r_qlen = S.r_id + n_redo, S.r_tlen = S.r_qlen + n_redo;
        S.r_rc = reinterpret_cast<uint8_t *>(S.r_tlen + n_redo), S.g_words = static_cast<uint32_t *>(ctx->sd_words.p);
        if ((rc = launch(SDK_PK_REDO_WRITE, n_pairs, n_tiles))) return rc;
        if ((rc = launch(SDK_PK_GATHER, n_redo, std::min<uint64_t>((2 * n_redo + SD_BLOCK / 64 - 1) / (SD_BLOCK / 64), 1u << 16)))) return rc;
        for (uint64_t a = 0; a < n_redo; a += SD_FB_PAIRS) {
            const uint64_t nb = std::min(SD_FB_PAIRS, n_redo - a);
            if ((rc = ensure(ctx, ctx->out_rec, nb * REC_WORDS * 4))) return rc;
            // CIGAR ops are merged runs: the host entry's first guess, (n+m)/4 + 8 per pair, run again once with what was needed
            uint64_t ops_cap = std::min<uint64_t>(16 * g_words, 2ull * fb_max * nb) / 4 + 8 * nb + 1024;
            for (int attempt = 0;; attempt++) {
                if ((rc = ensure(ctx, ctx->out_ops, ops_cap * 8))) return rc;
                uint64_t   needed = 0;
                BoundScope bound(ctx, max_score);  // (the full path stops and filters by it)
                rc = align_packed_device_impl(ctx, p, S.g_words, g_words, S.r_qoff + a, S.r_qlen + a, S.r_toff + a, S.r_tlen + a, nullptr, nb, fb_max,
                                              ctx->out_rec.p, ctx->out_ops.p, ops_cap, &needed, st);
                if (rc == WFAHIP_ERR_OOM && needed > ops_cap && attempt == 0) {
                    ops_cap = needed;
                    continue;
                }
                break;
            }
            if (rc) return rc;
            const wfahip_timing &f = ctx->timing;
            tm.kernel_ms += f.kernel_ms, tm.n_launches += f.n_launches, tm.arena_bytes = std::max(tm.arena_bytes, f.arena_bytes);
            if (!R.on_kernel && a == 0) tm.main_kernel_ms = f.main_kernel_ms, tm.n_main_launches = f.n_main_launches, tm.main_kernel_kind = f.main_kernel_kind;
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

extern "C" int wfahip_score_batch_packed_device(wfahip_ctx *ctx, const wfahip_params *p, const void *d_packed, uint64_t n_words,
                                                const void *d_q_woff, const void *d_q_len, const void *d_t_woff, const void *d_t_len,
                                                const void *d_q_rc, uint64_t n_pairs, uint32_t max_len, uint32_t max_score, void *d_status,
                                                void *d_score, void *stream) {
    WFAHIP_GUARD(score_batch_packed_device_impl(ctx, p, d_packed, n_words, d_q_woff, d_q_len, d_t_woff, d_t_len, d_q_rc, n_pairs, max_len, max_score,
                                                d_status, d_score, static_cast<hipStream_t>(stream)))
}

// ---- the survivors of a screen as the next stage's arrays (wfahip_select_pairs_device): a stable compaction of the pairs whose status is
// WFAHIP_PAIR_OK -- two launches of wfa_score_select_kernel with the scan between them, one fetch of the count.  The offsets are
// opaque: what comes out feeds wfahip_align_batch_packed_device or wfahip_align_batch_device as it is.
static int select_pairs_device_impl(wfahip_ctx *ctx, const void *d_status, uint64_t n_pairs, const void *d_q_off, const void *d_q_len,
                                    const void *d_t_off, const void *d_t_len, const void *d_q_rc, void *d_idx, void *d_q_off_out, void *d_q_len_out,
                                    void *d_t_off_out, void *d_t_len_out, void *d_q_rc_out, uint64_t *n_selected, hipStream_t st) {
    // (none of these checks dereferences ctx)
    if (!ctx || !n_selected) return WFAHIP_ERR_BAD_ARG;
    if (n_pairs && (!d_status || !d_q_off || !d_q_len || !d_t_off || !d_t_len || !d_q_off_out || !d_q_len_out || !d_t_off_out || !d_t_len_out))
        return WFAHIP_ERR_BAD_ARG;
    if ((d_q_rc == nullptr) != (d_q_rc_out == nullptr) || n_pairs > 0xFFFFFFF0ull) return WFAHIP_ERR_BAD_ARG;
    *n_selected = 0;
    if (n_pairs == 0) return WFAHIP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (!st) st = ctx->stream;
    const uint64_t n_tiles = (n_pairs + SD_TILE - 1) / SD_TILE;
    int            rc;
    if ((rc = ensure(ctx, ctx->sd_ctl, SDC_WORDS * 8))) return rc;
    if ((rc = ensure(ctx, ctx->sd_blk, n_tiles * sizeof(SDSum)))) return rc;
    SDParams S{};
    S.sel_status = static_cast<const int32_t *>(d_status), S.n = n_pairs;
    S.q_off = static_cast<const uint64_t *>(d_q_off), S.t_off = static_cast<const uint64_t *>(d_t_off);
    S.q_len = static_cast<const uint32_t *>(d_q_len), S.t_len = static_cast<const uint32_t *>(d_t_len), S.q_rc = static_cast<const uint8_t *>(d_q_rc);
    S.r_id = static_cast<uint32_t *>(d_idx), S.r_qoff = static_cast<uint64_t *>(d_q_off_out), S.r_toff = static_cast<uint64_t *>(d_t_off_out);
    S.r_qlen = static_cast<uint32_t *>(d_q_len_out), S.r_tlen = static_cast<uint32_t *>(d_t_len_out), S.r_rc = static_cast<uint8_t *>(d_q_rc_out);
    S.ctl = static_cast<unsigned long long *>(ctx->sd_ctl.p), S.blk = static_cast<SDSum *>(ctx->sd_blk.p);
    HIP_TRY(wfa_launch_score_dev(SDK_SELECT_COUNT, S, (uint32_t)n_tiles, st));
    SDParams T = S;
    T.n = n_tiles, T.c_cnt = SDC_N_REDO, T.c_wt = SDC_REDO_SUM;
    HIP_TRY(wfa_launch_score_dev(SDK_SCAN, T, 1, st));
    HIP_TRY(wfa_launch_score_dev(SDK_SELECT_WRITE, S, (uint32_t)n_tiles, st));
    // (through the context's pinned block: a pageable copy of 64 bytes costs 0.3 ms)
    HIP_TRY(hipMemcpyAsync(ctx->hpin + HPIN_CTRL, S.ctl, SDC_WORDS * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    uint64_t hc[SDC_WORDS];
    std::memcpy(hc, ctx->hpin + HPIN_CTRL, SDC_WORDS * 8);
    *n_selected = hc[SDC_N_REDO];
    return WFAHIP_OK;
}

extern "C" int wfahip_select_pairs_device(wfahip_ctx *ctx, const void *d_status, uint64_t n_pairs, const void *d_q_off, const void *d_q_len,
                                          const void *d_t_off, const void *d_t_len, const void *d_q_rc, void *d_idx, void *d_q_off_out,
                                          void *d_q_len_out, void *d_t_off_out, void *d_t_len_out, void *d_q_rc_out, uint64_t *n_selected,
                                          void *stream) {
    WFAHIP_GUARD(select_pairs_device_impl(ctx, d_status, n_pairs, d_q_off, d_q_len, d_t_off, d_t_len, d_q_rc, d_idx, d_q_off_out, d_q_len_out,
                                          d_t_off_out, d_t_len_out, d_q_rc_out, n_selected, static_cast<hipStream_t>(stream)))
}

// ---- score matrix (wfahip_score_matrix): every query against every target, score only.  The n_q + n_t sequences are packed and
// flagged once (host threads, pack_seq_fast) and uploaded as one table of 2-bit words; the matrix instances of the score kernels
// take the cells of a rectangular tile, a workgroup per cell, and stage the cell's two sequences from the table.  Tiles are
// double-buffered: tile c downloads on stream2 while tile c + 1 runs, and the host scatters it into the caller's arrays.  What the
// kernels hand back goes through the full path of wfahip_align_batch, in batches of MX_FB_PAIRS cells.
// wfahip_score_matrix_rc is the same entry with a flag per query ROW: every cell of a flagged row scores the reverse complement of its query.
// The table still holds every sequence once, forward (with the same arrays on both sides a sequence is a target too): the kernels read the
// row's flag with the cell (mx_cell) and reverse-complement the query's words as they stage them; flagged long rows are written once
// behind the table's words, P.mx_rc_shift words behind their forward form (wfa_rc_words_kernel); the cells the kernels hand back take the
// full path on bytes reverse-complemented here (rc_byte).
namespace {
// the complement of a byte: A <-> T, C <-> G in either case, every other byte itself
inline uint8_t rc_byte(uint8_t c) {
    switch (c) {
    case 'A': return 'T';
    case 'T': return 'A';
    case 'C': return 'G';
    case 'G': return 'C';
    case 'a': return 't';
    case 't': return 'a';
    case 'c': return 'g';
    case 'g': return 'c';
    }
    return c;
}
}  // namespace

static int score_matrix_impl(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *seq_blob, uint64_t blob_bytes, const uint64_t *q_off,
                             const uint32_t *q_len, uint64_t n_q, const uint8_t *q_rc, const uint64_t *t_off, const uint32_t *t_len, uint64_t n_t,
                             uint32_t max_score, int32_t *status, uint32_t *score, uint64_t out_stride) {
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
    q_rc = any_flag(q_rc, n_q);
    wfahip_timing tm{};
    const auto    put = [&](uint64_t i, uint64_t j, uint32_t st, uint32_t sc) {
        status[i * stride + j] = (int32_t)st, score[i * stride + j] = st == ST_OK ? sc : 0u;
    };
    KParams               P{};
    const ScoreRoute      R = score_route(P, p);
    const bool            glob = R.glob;
    std::vector<uint64_t> fb;  // cells (i * n_t + j) the kernels handed back
    if (R.on_kernel) {
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
        parallel_ranges(0, n_seq, (unsigned)std::min<uint64_t>(host_pack_threads(16, false), n_seq / 4096 + 1), [&](uint64_t a, uint64_t b) {
            for (uint64_t s = a; s < b; s++) {
                if (!(seq[s].w == 0u || (use_long && seq[s].w == MXF_LONG))) continue;
                const uint8_t *src = seq_blob + (s < n_q ? q_off[s] : t_off[s - n_q]);
                if (pack_seq_fast(src, seq[s].z, words.data() + ((uint64_t)seq[s].y << 32 | seq[s].x))) seq[s].w |= MXF_BYTES;
            }
        });
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
        // the flagged rows with a cell for the long kernel -- a long row, or a row of any length when a column is long: the kernel takes every
        // cell with a long side -- : their reverse complements go behind the table's words, each as far behind its forward form as the first
        // of them (words [lo, hi) of the table -> [words.size(), ..)); a job of wfa_rc_words_kernel per row.  (Rows with a byte outside
        // ACGT have no such cell.)  The span costs at most the table's words again on the device, nothing on the host or the bus
        std::vector<uint4> jobs;
        uint64_t           rc_lo = UINT64_MAX, rc_hi = 0;
        bool               long_col = false;
        for (uint64_t s = same ? 0 : n_q; s < n_seq && use_long && q_rc; s++) long_col |= seq[s].w == MXF_LONG;
        const auto wants_rc = [&](uint64_t s) { return q_rc[s] && (seq[s].w == MXF_LONG || (seq[s].w == 0u && long_col)); };
        for (uint64_t s = 0; s < n_q && use_long && q_rc; s++) {
            if (!wants_rc(s)) continue;
            const uint64_t w = (uint64_t)seq[s].y << 32 | seq[s].x;
            rc_lo = std::min(rc_lo, w), rc_hi = std::max(rc_hi, w + wfahip_packed_words(seq[s].z));
        }
        if (rc_hi) {
            P.mx_rc_shift = words.size() - rc_lo;
            for (uint64_t s = 0; s < n_q; s++) {
                if (!wants_rc(s)) continue;
                const uint64_t d = ((uint64_t)seq[s].y << 32 | seq[s].x) + P.mx_rc_shift;
                jobs.push_back(make_uint4(seq[s].x, seq[s].y, seq[s].z, 0u));
                jobs.push_back(make_uint4((uint32_t)d, (uint32_t)(d >> 32), 0u, 0u));
            }
        }
        if ((rc = ensure(ctx, ctx->mx_seq, n_seq * 16))) return rc;
        if ((rc = ensure(ctx, ctx->mx_words, (words.size() + (rc_hi ? rc_hi - rc_lo + 4 : 0)) * 4))) return rc;
        HIP_TRY(hipMemcpyAsync(ctx->mx_seq.p, seq.data(), n_seq * 16, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ctx->mx_words.p, words.data(), words.size() * 4, hipMemcpyHostToDevice, st));
        if (q_rc) {
            if ((rc = ensure(ctx, ctx->in_rc, n_q))) return rc;
            HIP_TRY(hipMemcpyAsync(ctx->in_rc.p, q_rc, n_q, hipMemcpyHostToDevice, st));
            P.q_rc = static_cast<const uint8_t *>(ctx->in_rc.p);
        }
        if (!jobs.empty()) {
            if ((rc = ensure(ctx, ctx->rc_jobs, jobs.size() * 16))) return rc;
            HIP_TRY(hipMemcpyAsync(ctx->rc_jobs.p, jobs.data(), jobs.size() * 16, hipMemcpyHostToDevice, st));
        }
        P.mx_seq = static_cast<const uint4 *>(ctx->mx_seq.p), P.mx_words = static_cast<const uint32_t *>(ctx->mx_words.p);
        P.mx_tbase = same ? 0u : n_q;
        P.max_score = max_score;
        // ---- tiles: C targets x R queries, at most `tile` cells (columns split as well: 1 x 1e8 is 24 tiles)
        uint64_t tile = glob ? MX_TILE_GLOBAL : std::min<uint64_t>(1ull << 18, MX_CKPT_BYTES / (WIDE_CKPT_WORDS * 4ull));
        if (ctx->opt_matrix_tile_cells > 0) tile = std::min<uint64_t>((uint64_t)ctx->opt_matrix_tile_cells, 1ull << 24);
        const uint64_t C = std::min(n_t, tile), Rq = std::min(n_q, tile / C);
        tile = Rq * C;
        ScoreGeom G;
        if ((rc = score_geometry(ctx, P, L, tile, G))) return rc;
        if ((rc = ensure(ctx, ctx->mx_out, (size_t)tile * 16))) return rc;
        HIP_TRY(grow_pinned(ctx->mx_pin, ctx->mx_pin_bytes, (size_t)tile * 16, 0));
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
        if (!jobs.empty()) {
            HIP_TRY(wfa_launch_rc_words(static_cast<const uint4 *>(ctx->rc_jobs.p), static_cast<uint32_t *>(ctx->mx_words.p), (uint32_t)(jobs.size() / 2), st));
            tm.n_launches++;
        }
        Tile     prev{};
        uint64_t c = 0;
        for (uint64_t r0 = 0; r0 < n_q; r0 += Rq)
            for (uint64_t c0 = 0; c0 < n_t; c0 += C, c++) {
                const Tile t{r0, c0, std::min(Rq, n_q - r0), std::min(C, n_t - c0)};
                const int  b = (int)(c & 1u);
                if (c >= 2) HIP_TRY(hipStreamWaitEvent(st, ctx->mx_ev[2 + b], 0));  // (buffer b's previous tile has left the device)
                const uint32_t cn = (uint32_t)(t.rr * t.cc);
                P.score_out = dout + (uint64_t)b * tile, P.chunk_first = 0u, P.chunk_n = cn;
                P.mx_r0 = t.r0, P.mx_c0 = t.c0, P.mx_cols = (uint32_t)t.cc;
                // (a global tile with long sequences: two launches over it, each kernel takes its own cells and leaves the other's slots alone)
                bool some_long = false, all_long = false;
                if (use_long) {
                    const uint64_t tb = same ? 0u : n_q;
                    const uint64_t lr = n_lng[t.r0 + t.rr] - n_lng[t.r0], lc = n_lng[tb + t.c0 + t.cc] - n_lng[tb + t.c0];
                    some_long = lr != 0 || lc != 0, all_long = lr == t.rr || lc == t.cc;
                }
                if (!all_long && (rc = score_launch_short(ctx, STAGE_MATRIX, R, G, P, st, tm))) return rc;
                if (some_long) {
                    KParams PL = P;
                    PL.lds_seq_words = score_long_window(ctx->opt_score_long_window);
                    HIP_TRY(wfa_launch_score_long(true, PL, cn, (size_t)score_long_lds_words(PL.lds_seq_words) * 4, st));
                    tm.n_launches++;
                    if (all_long) tm.n_main_launches++;  // (one main launch per tile)
                }
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
        tm.main_kernel_kind = glob ? (long_main ? K_MATRIX_LONG : K_MATRIX) : K_MATRIX_WIDE;
    }
    // ---- the full path: what the kernels handed back -- or every cell, for a penalty shape without an instance -- a batch of at most
    // MX_FB_PAIRS cells at a time
    const uint64_t n_fb = R.on_kernel ? (uint64_t)fb.size() : n_q * n_t;
    // (the flagged rows among them: the full path reads their queries from a copy of the blob with their reverse complements appended --
    // align_batch_entry takes ONE blob, so while such cells are aligned the host holds the blob a second time, plus those rows)
    std::vector<uint8_t>  rblob;
    std::vector<uint64_t> rq_off;
    if (q_rc && n_fb) {
        std::vector<uint8_t> need(n_q, 0);
        for (uint64_t k = 0; k < n_fb; k++) {
            const uint64_t i = (R.on_kernel ? fb[k] : k) / n_t;
            need[i] = q_rc[i] && q_len[i] && q_len[i] <= WFAHIP_MAX_SEQ_LEN;
        }
        rblob.assign(seq_blob, seq_blob + blob_bytes), rq_off.assign(q_off, q_off + n_q);
        for (uint64_t i = 0; i < n_q; i++) {
            if (!need[i]) continue;
            rq_off[i] = rblob.size();
            const uint8_t *const src = seq_blob + q_off[i];
            for (uint32_t b = q_len[i]; b-- > 0;) rblob.push_back(rc_byte(src[b]));
        }
        seq_blob = rblob.data(), blob_bytes = rblob.size(), q_off = rq_off.data();
    }
    for (uint64_t a = 0; a < n_fb; a += MX_FB_PAIRS) {
        const auto cell = [&](uint64_t k) {
            const uint64_t x = R.on_kernel ? fb[a + k] : a + k;
            return std::make_pair(x / n_t, x % n_t);
        };
        if ((rc = score_fallback(ctx, p, seq_blob, blob_bytes, q_off, q_len, t_off, t_len, std::min(MX_FB_PAIRS, n_fb - a), max_score, R.on_kernel, tm,
                                 cell, [&](uint64_t k, uint32_t st, uint32_t sc) {
                                     const auto ij = cell(k);
                                     put(ij.first, ij.second, st, sc);
                                 })))
            return rc;
    }
    tm.n_retried_pairs = (uint32_t)std::min<uint64_t>(n_fb, UINT32_MAX);
    tm.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    ctx->timing = tm;
    return WFAHIP_OK;
}

extern "C" int wfahip_score_matrix(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *seq_blob, uint64_t blob_bytes, const uint64_t *q_off,
                                   const uint32_t *q_len, uint64_t n_q, const uint64_t *t_off, const uint32_t *t_len, uint64_t n_t, uint32_t max_score,
                                   int32_t *status, uint32_t *score, uint64_t out_stride) {
    WFAHIP_GUARD(score_matrix_impl(ctx, p, seq_blob, blob_bytes, q_off, q_len, n_q, nullptr, t_off, t_len, n_t, max_score, status, score, out_stride))
}
extern "C" int wfahip_score_matrix_rc(wfahip_ctx *ctx, const wfahip_params *p, const uint8_t *seq_blob, uint64_t blob_bytes, const uint64_t *q_off,
                                      const uint32_t *q_len, uint64_t n_q, const uint8_t *q_rc, const uint64_t *t_off, const uint32_t *t_len, uint64_t n_t,
                                      uint32_t max_score, int32_t *status, uint32_t *score, uint64_t out_stride) {
    WFAHIP_GUARD(score_matrix_impl(ctx, p, seq_blob, blob_bytes, q_off, q_len, n_q, q_rc, t_off, t_len, n_t, max_score, status, score, out_stride))
}
