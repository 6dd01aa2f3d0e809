// wfa_wide_pk.hip -- translation unit of what the length-class routing of semi-global batches (align_device, wfa_host.hip) adds to
// wfa_wide_kernel's byte instances: the full-alignment instances with the packed prologue (STAGE_PACKED: the host entries with packed
// input, wfahip_align_batch_packed and the autopacked wfahip_align_batch) and the plan kernels (wfa_wide_plan.hpp).  The launches
// below are declared for the router in wfa_ctx.hpp.
#define WFA_NO_AUX_KERNELS 1
#define WFA_WIDE_PLAN_UNIT 1
#include "wfa_wide.hpp"
#include "wfa_wide_plan.hpp"
#include "wfa_fwd.hpp"  // WFA_FWD_SHAPES

namespace wfa {

// wfa_wide_kernel<.., SCORE = false, STAGE_PACKED> of penalty shape `shape`: as wfa_launch_wide (wfa_host.hip) launches the byte instances
hipError_t wfa_launch_wide_packed(int shape, int phase, int waves, const KParams &P, uint32_t grid, size_t lds_bytes, hipStream_t st) {
    const auto go = [&](auto kern, int nw) { return wfa_launch_wide_instance(kern, nw, P, grid, lds_bytes, st); };
#define WFA_WIDE_PK_SHAPE(I, tag, DX_, DOE_)                                                                    \
    case 3 * I: return go(wfa_wide_kernel<DX_, DOE_, 0, 1, false, STAGE_PACKED>, 1);                           \
    case 3 * I + 1: return go(wfa_wide_kernel<DX_, DOE_, 0, 4, false, STAGE_PACKED>, 4);                       \
    case 3 * I + 2: return go(wfa_wide_kernel<DX_, DOE_, 1, 1, false, STAGE_PACKED>, 1);
    switch (shape * 3 + (phase ? 2 : (waves > 1 ? 1 : 0))) {
        WFA_FWD_SHAPES(WFA_WIDE_PK_SHAPE)
    }
#undef WFA_WIDE_PK_SHAPE
    return hipErrorInvalidValue;
}

// the three launches of the plan, in order, on `st`; S.ctl zeroed first.  S.ids == nullptr: count and scan alone
hipError_t wfa_launch_wide_plan(const WPParams &S, hipStream_t st) {
    hipError_t e = hipMemsetAsync(S.ctl, 0, WPC_WORDS * 4, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(wfa_wide_plan_count_kernel, dim3(S.tiles), dim3(WP_BLOCK), 0, st, S);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(wfa_wide_plan_scan_kernel, dim3(1), dim3(WP_BLOCK), 0, st, S);
    if ((e = hipGetLastError()) != hipSuccess || !S.ids) return e;
    hipLaunchKernelGGL(wfa_wide_plan_scatter_kernel, dim3(S.tiles), dim3(WP_BLOCK), 0, st, S);
    return hipGetLastError();
}

}  // namespace wfa
