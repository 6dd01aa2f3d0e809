// wfa_fwd.hpp -- launchers of the sub-wave forward kernels (wfa_blk_kernel, wfa_lane_kernel, wfa_duo_kernel), one
// translation unit per PENALTY SHAPE.
//
// The reference takes any penalties (wfa.go:32-36).  What the register-ring kernels are built around is not the penalties
// but their shape in units of g = gcd(x, o+e, e): DX = x/g and DOE = (o+e)/g say how many score steps back M[s-x] and
// M[s-o-e] lie (wfa.go:557-560), and with e/g == 1 the I and D sources are the previous row.  Rounds 1-4 had the one
// shape of the default penalties, 2 : 4 (4/6/2 and its multiples, 2/3/1); everything else ran on the LDS-ring kernel
// (wfa_packed_kernel, any shape, ring depth a run-time value) or the one-workgroup-per-pair kernel.  Round 5 instantiates the
// same kernels per shape (template arguments DX, DOE: the M ring holds max(DX, DOE) rows and the step loop is unrolled
// that many times), each shape in a translation unit of its own (wfa_fwd_s<DX><DOE>.hip includes wfa_fwd_shape.inc) so
// that they compile side by side:
//     2 : 4   4/6/2 (default), 2/3/1, 8/12/4      1 : 3   2/4/2
//     1 : 2   1/1/1, 2/2/2                          2 : 3   4/4/2, 2/2/1
//     2 : 2   4/2/2, 2/1/1                          3 : 3   6/4/2 (x == o+e)
// Shapes without an instance (e/g != 1, a ring deeper than four rows) keep the LDS-ring kernel.
#pragma once
#include "wfa_common.hpp"
#include "wfa_kinds.hpp"

namespace wfa {

// the shapes with instances: X(index, tag, DX, DOE).  fwd_shape(), the per-shape entry points below and every switch over a
// shape index (wfa_host.hip, wfa_duo.hip, wfa_score.hip, wfa_wide_pk.hip) are generated from this list, in this order
#define WFA_FWD_SHAPES(X) X(0, s24, 2, 4) X(1, s13, 1, 3) X(2, s12, 1, 2) X(3, s23, 2, 3) X(4, s22, 2, 2) X(5, s33, 3, 3)

constexpr int FWD_N_SHAPES = 6;
// index of the shape's instances, -1: none
inline int fwd_shape(uint32_t dx, uint32_t doe, uint32_t de) {
    if (de != 1u) return -1;
#define WFA_FWD_SHAPE_IS(I, tag, DX_, DOE_) \
    if (dx == DX_##u && doe == DOE_##u) return I;
    WFA_FWD_SHAPES(WFA_FWD_SHAPE_IS)
#undef WFA_FWD_SHAPE_IS
    return -1;
}

// flags of wfa_launch_fwd
enum : uint32_t {
    FWD_CENSUS   = 1u,  // count the stored wavefront words (REC_CELLS)
    FWD_STREAM   = 2u,  // K_BLK16 only, shape 2 : 4 only: the launch also walks the backtrace of finished pairs
    FWD_BATCH    = 4u,  // K_BLK16 / K_NARROW: a group stages BLK_BATCH queue entries per refill (short reads)
    FWD_ADAPTIVE = 8u   // K_LANE: the instance that tracks wf-adaptive's distances
};

// Forward kernel of `kind` (wfa_kinds.hpp: K_BLK16 .. K_LONE128 without K_TEAM and K_DUO) for penalty shape `shape`.
// hipErrorInvalidValue: no such instance.
hipError_t wfa_launch_fwd(int shape, int kind, uint32_t flags, const KParams &P, uint32_t grid, size_t lds_bytes, hipStream_t st);

// wfahip_align_pair's lone-pair instance (a lane per diagonal, the wave walks its own backtrace): lds_arena = the rows in LDS
hipError_t wfa_launch_pair(int shape, bool lds_arena, const KParams &P, size_t lds_bytes, hipStream_t st);

// one wfa_wide_kernel instance with `waves` waves per pair; rings above 64 KB need the opt-in (per device: the attribute belongs
// to the kernel as loaded there)
template <class K>
hipError_t wfa_launch_wide_instance(K kern, int waves, const KParams &P, uint32_t grid, size_t lds_bytes, hipStream_t st) {
    if (lds_bytes > 64 * 1024)
        if (const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * waves), lds_bytes, st, P);
    return hipGetLastError();
}

// per-shape entry points (wfa_fwd_s*.hip)
#define WFA_FWD_DECL(I, tag, DX_, DOE_)                                                                                     \
    hipError_t wfa_launch_fwd_##tag(int kind, uint32_t flags, const KParams &P, uint32_t grid, size_t lds_bytes, hipStream_t st); \
    hipError_t wfa_launch_pair_##tag(bool lds_arena, const KParams &P, size_t lds_bytes, hipStream_t st);
WFA_FWD_SHAPES(WFA_FWD_DECL)
#undef WFA_FWD_DECL

}  // namespace wfa
