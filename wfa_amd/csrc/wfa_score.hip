// wfa_score.hip -- translation unit of the score-only kernels behind wfahip_score_batch: wfa_score_kernel (global pairs, any
// penalty shape score_shape_ok() takes; wfa_score_long_kernel for reads beyond its 2 047 bases) and the score instances of wfa_wide_kernel (semi-global pairs, the shapes of
// wfa_fwd_shape.inc), their matrix instances behind wfahip_score_matrix and their packed pair-list instances behind
// wfahip_score_batch_packed; and the routing kernels of wfahip_score_batch_device, wfahip_score_batch_packed_device and wfahip_select_pairs_device
// (wfa_score_dev.hpp).  The routers are wfa_score_entry.hip (score_batch_impl, score_batch_device_impl, score_matrix_impl); the
// launches below are declared for them in wfa_ctx.hpp.
#define WFA_NO_AUX_KERNELS 1
#define WFA_SCORE_UNIT 1
#include "wfa_wide.hpp"
#include "wfa_score.hpp"
#include "wfa_score_long.hpp"
#include "wfa_score_dev.hpp"
#include "wfa_fwd.hpp"  // WFA_FWD_SHAPES

namespace wfa {

// (STAGE_MATRIX: the instances of wfahip_score_matrix -- a cell of the score matrix per workgroup; STAGE_PACKED: those of
// wfahip_score_batch_packed -- a pair of a list over caller-packed words; wfa_matrix.hpp)
template <int STAGE>
static hipError_t launch_score(const KParams &P, uint32_t grid, size_t lds_bytes, hipStream_t st) {
    if (lds_bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(wfa_score_kernel<STAGE>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(wfa_score_kernel<STAGE>, dim3(grid), dim3(64), lds_bytes, st, P);
    return hipGetLastError();
}

// wfa_score_long_kernel (wfa_score_long.hpp) over a list of `grid` long pairs -- matrix: over the `grid` cells of a tile, of which it
// takes those with a long sequence.  Its LDS (score_long_lds_words: 14 KB at the default window, 44 KB at the largest) needs no opt-in
hipError_t wfa_launch_score_long(bool matrix, const KParams &P, uint32_t grid, size_t lds_bytes, hipStream_t st) {
    if (matrix)
        hipLaunchKernelGGL(wfa_score_long_kernel<true>, dim3(grid), dim3(64), lds_bytes, st, P);
    else
        hipLaunchKernelGGL(wfa_score_long_kernel<false>, dim3(grid), dim3(64), lds_bytes, st, P);
    return hipGetLastError();
}

// wfa_rc_words_kernel (wfa_score_long.hpp): the reverse complements of `n_jobs` flagged long queries, from and into `words`
hipError_t wfa_launch_rc_words(const uint4 *jobs, uint32_t *words, uint32_t n_jobs, hipStream_t st) {
    hipLaunchKernelGGL(wfa_rc_words_kernel, dim3(n_jobs), dim3(256), 0, st, jobs, words, n_jobs);
    return hipGetLastError();
}

// wfa_wide_kernel<.., SCORE = true> of penalty shape `shape` (wfa_fwd.hpp: fwd_shape()): phase 0 with `waves` waves per pair (1 or 4),
// phase 1 with one -- as wfa_launch_wide (wfa_host.hip) launches the full-path instances
template <int STAGE>
static hipError_t launch_wide_score(int shape, int phase, int waves, const KParams &P, uint32_t grid, size_t lds_bytes, hipStream_t st) {
    const auto go = [&](auto kern, int nw) { return wfa_launch_wide_instance(kern, nw, P, grid, lds_bytes, st); };
#define WFA_WIDE_SCORE_SHAPE(I, tag, DX_, DOE_)                                                                 \
    case 3 * I: return go(wfa_wide_kernel<DX_, DOE_, 0, 1, true, STAGE>, 1);                                   \
    case 3 * I + 1: return go(wfa_wide_kernel<DX_, DOE_, 0, 4, true, STAGE>, 4);                               \
    case 3 * I + 2: return go(wfa_wide_kernel<DX_, DOE_, 1, 1, true, STAGE>, 1);
    switch (shape * 3 + (phase ? 2 : (waves > 1 ? 1 : 0))) {
        WFA_FWD_SHAPES(WFA_WIDE_SCORE_SHAPE)
    }
#undef WFA_WIDE_SCORE_SHAPE
    return hipErrorInvalidValue;
}

// (instantiated in this order, so that the kernels keep their places in the code object: the batch instances, then the matrix ones,
// then the packed pair-list ones)
template hipError_t launch_score<STAGE_BYTES>(const KParams &, uint32_t, size_t, hipStream_t);
template hipError_t launch_wide_score<STAGE_BYTES>(int, int, int, const KParams &, uint32_t, size_t, hipStream_t);
template hipError_t launch_score<STAGE_MATRIX>(const KParams &, uint32_t, size_t, hipStream_t);
template hipError_t launch_wide_score<STAGE_MATRIX>(int, int, int, const KParams &, uint32_t, size_t, hipStream_t);
template hipError_t launch_score<STAGE_PACKED>(const KParams &, uint32_t, size_t, hipStream_t);
template hipError_t launch_wide_score<STAGE_PACKED>(int, int, int, const KParams &, uint32_t, size_t, hipStream_t);

hipError_t wfa_launch_score(int stage, const KParams &P, uint32_t grid, size_t lds_bytes, hipStream_t st) {
    switch (stage) {
    case STAGE_BYTES: return launch_score<STAGE_BYTES>(P, grid, lds_bytes, st);
    case STAGE_MATRIX: return launch_score<STAGE_MATRIX>(P, grid, lds_bytes, st);
    case STAGE_PACKED: return launch_score<STAGE_PACKED>(P, grid, lds_bytes, st);
    }
    return hipErrorInvalidValue;
}
hipError_t wfa_launch_wide_score(int stage, int shape, int phase, int waves, const KParams &P, uint32_t grid, size_t lds_bytes, hipStream_t st) {
    switch (stage) {
    case STAGE_BYTES: return launch_wide_score<STAGE_BYTES>(shape, phase, waves, P, grid, lds_bytes, st);
    case STAGE_MATRIX: return launch_wide_score<STAGE_MATRIX>(shape, phase, waves, P, grid, lds_bytes, st);
    case STAGE_PACKED: return launch_wide_score<STAGE_PACKED>(shape, phase, waves, P, grid, lds_bytes, st);
    }
    return hipErrorInvalidValue;
}

// the routing kernels of wfahip_score_batch_device, wfahip_score_batch_packed_device and wfahip_select_pairs_device (wfa_score_dev.hpp): kernel `k` (SDK_*) over `grid` workgroups of SD_BLOCK threads
hipError_t wfa_launch_score_dev(int k, const SDParams &S, uint32_t grid, hipStream_t st) {
    const dim3 g(grid), b(SD_BLOCK);
    switch (k) {
    case SDK_PLAN_COUNT: hipLaunchKernelGGL(wfa_score_plan_kernel<false>, g, b, 0, st, S); break;
    case SDK_PLAN_WRITE: hipLaunchKernelGGL(wfa_score_plan_kernel<true>, g, b, 0, st, S); break;
    case SDK_SCAN: hipLaunchKernelGGL(wfa_score_scan_kernel, dim3(1), b, 0, st, S); break;
    case SDK_PACK: hipLaunchKernelGGL(wfa_score_pack_kernel, g, b, 0, st, S); break;
    case SDK_LIST_COUNT: hipLaunchKernelGGL(wfa_score_list_kernel<false>, g, b, 0, st, S); break;
    case SDK_LIST_WRITE: hipLaunchKernelGGL(wfa_score_list_kernel<true>, g, b, 0, st, S); break;
    case SDK_REDO_COUNT: hipLaunchKernelGGL(wfa_score_redo_kernel<false>, g, b, 0, st, S); break;
    case SDK_REDO_WRITE: hipLaunchKernelGGL(wfa_score_redo_kernel<true>, g, b, 0, st, S); break;
    case SDK_FINISH: hipLaunchKernelGGL(wfa_score_finish_kernel, g, b, 0, st, S); break;
    case SDK_PK_PLAN_COUNT: hipLaunchKernelGGL(wfa_score_pkplan_kernel<false>, g, b, 0, st, S); break;
    case SDK_PK_PLAN_WRITE: hipLaunchKernelGGL(wfa_score_pkplan_kernel<true>, g, b, 0, st, S); break;
    case SDK_PK_RCQ: hipLaunchKernelGGL(wfa_score_rcq_kernel, g, b, 0, st, S); break;
    case SDK_PK_REDO_COUNT: hipLaunchKernelGGL(wfa_score_pkredo_kernel<false>, g, b, 0, st, S); break;
    case SDK_PK_REDO_WRITE: hipLaunchKernelGGL(wfa_score_pkredo_kernel<true>, g, b, 0, st, S); break;
    case SDK_PK_GATHER: hipLaunchKernelGGL(wfa_score_gather_kernel, g, b, 0, st, S); break;
    case SDK_SELECT_COUNT: hipLaunchKernelGGL(wfa_score_select_kernel<false>, g, b, 0, st, S); break;
    case SDK_SELECT_WRITE: hipLaunchKernelGGL(wfa_score_select_kernel<true>, g, b, 0, st, S); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace wfa
