// wfa_fwd_shape.inc -- body of a per-shape translation unit (wfa_fwd.hpp).  The including file defines WFA_SHAPE_DX,
// WFA_SHAPE_DOE and WFA_SHAPE_TAG (s24, s13, ..).  Only the shape of the default penalties carries the instances that exist
// for experiments and comparisons (the streaming backtrace, the 8-lane unbatched forms, round 3's single-pair paths).
#define WFA_NO_AUX_KERNELS 1
#include <atomic>
#include "wfa_blk.hpp"
#include "wfa_lane.hpp"
#include "wfa_fwd.hpp"

#define WFA_CAT2(a, b) a##b
#define WFA_CAT(a, b) WFA_CAT2(a, b)

namespace wfa {

namespace {
constexpr int  SDX = WFA_SHAPE_DX, SDOE = WFA_SHAPE_DOE;
constexpr bool DEFAULT_SHAPE = SDX == 2 && SDOE == 4;

template <int G, int BATCH, bool STREAM, int PPT, bool CENSUS, bool LONG, bool LDSA = false>
hipError_t go(const KParams &P, uint32_t grid, size_t lds_bytes, hipStream_t st) {
    hipLaunchKernelGGL((wfa_blk_kernel<G, BATCH, STREAM, PPT, CENSUS, LONG, LDSA, SDX, SDOE>), dim3(grid), dim3(64), lds_bytes, st, P);
    return hipGetLastError();
}
template <bool CENSUS, bool ADAPTIVE>
hipError_t go_lane(const KParams &P, uint32_t grid, size_t lds_bytes, hipStream_t st) {
    if constexpr (SDX <= SDOE) {
        hipLaunchKernelGGL((wfa_lane_kernel<CENSUS, ADAPTIVE, SDX, SDOE>), dim3(grid), dim3(64), lds_bytes, st, P);
        return hipGetLastError();
    } else {
        return hipErrorInvalidValue;
    }
}
}  // namespace

hipError_t WFA_CAT(wfa_launch_fwd_, WFA_SHAPE_TAG)(int kind, uint32_t flags, const KParams &P, uint32_t grid, size_t lds_bytes, hipStream_t st) {
    const bool census = (flags & FWD_CENSUS) != 0u, stream = (flags & FWD_STREAM) != 0u, batch = (flags & FWD_BATCH) != 0u;
    const bool adaptive = (flags & FWD_ADAPTIVE) != 0u;
    switch (kind) {
    case K_BLK16:  // four pairs per wave, 64 diagonals
        if (batch) return go<16, BLK_BATCH, false, 0, true, false>(P, grid, lds_bytes, st);
        if constexpr (DEFAULT_SHAPE) {
            if (stream) return census ? go<16, 1, true, 0, true, false>(P, grid, lds_bytes, st) : go<16, 1, true, 0, false, false>(P, grid, lds_bytes, st);
        } else if (stream) {
            return hipErrorInvalidValue;
        }
        return census ? go<16, 1, false, 0, true, false>(P, grid, lds_bytes, st) : go<16, 1, false, 0, false, false>(P, grid, lds_bytes, st);
    case K_BLK8:  // eight pairs per wave, eight diagonals per lane (option blk = 8)
        if constexpr (DEFAULT_SHAPE) return go<8, 1, false, 0, true, false>(P, grid, lds_bytes, st);
        return hipErrorInvalidValue;
    case K_BLK64:  // a wave per pair, 256 diagonals
        return go<64, 1, false, 0, true, false>(P, grid, lds_bytes, st);
    case K_NARROW:  // eight pairs per wave, 32 diagonals (short reads)
        if (batch) return census ? go<8, BLK_BATCH, false, 4, true, false>(P, grid, lds_bytes, st) : go<8, BLK_BATCH, false, 4, false, false>(P, grid, lds_bytes, st);
        if constexpr (DEFAULT_SHAPE) return go<8, 1, false, 4, true, false>(P, grid, lds_bytes, st);
        return hipErrorInvalidValue;
    case K_BLK32:  // two pairs per wave, 128 diagonals
        return go<32, 1, false, 0, true, false>(P, grid, lds_bytes, st);
    case K_LANE:  // a lane per pair (short reads)
        if (census) return adaptive ? go_lane<true, true>(P, grid, lds_bytes, st) : go_lane<true, false>(P, grid, lds_bytes, st);
        return adaptive ? go_lane<false, true>(P, grid, lds_bytes, st) : go_lane<false, false>(P, grid, lds_bytes, st);
    // long reads: the same groups with sliding sequence windows
    case K_LONG16: return census ? go<16, 1, false, 0, true, true>(P, grid, lds_bytes, st) : go<16, 1, false, 0, false, true>(P, grid, lds_bytes, st);
    case K_LONG32: return go<32, 1, false, 0, true, true>(P, grid, lds_bytes, st);
    case K_LONG64: return census ? go<64, 1, false, 0, true, true>(P, grid, lds_bytes, st) : go<64, 1, false, 0, false, true>(P, grid, lds_bytes, st);
    case K_LONE64: return census ? go<64, 1, false, 1, true, true>(P, grid, lds_bytes, st) : go<64, 1, false, 1, false, true>(P, grid, lds_bytes, st);
    case K_LONE128: return census ? go<64, 1, false, 2, true, true>(P, grid, lds_bytes, st) : go<64, 1, false, 2, false, true>(P, grid, lds_bytes, st);
    }
    return hipErrorInvalidValue;
}

hipError_t WFA_CAT(wfa_launch_pair_, WFA_SHAPE_TAG)(bool lds_arena, const KParams &P, size_t lds_bytes, hipStream_t st) {
    if (lds_arena) {
        const auto kern = wfa_blk_kernel<64, 1, false, 1, false, false, true, SDX, SDOE>;
        // the attribute belongs to the kernel AS LOADED ON ONE DEVICE: one bit per device (contexts of several GPUs in one process:
        // wfahip_create_multi), set from any host thread
        static std::atomic<uint64_t> attr_set{0};
        int dev = 0;
        if (const hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
        const uint64_t bit = 1ull << (dev & 63);
        if ((attr_set.load(std::memory_order_acquire) & bit) == 0 || dev >= 64) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            if (e != hipSuccess) return e;
            attr_set.fetch_or(bit, std::memory_order_release);
        }
        hipLaunchKernelGGL(kern, dim3(1), dim3(64), lds_bytes, st, P);
        return hipGetLastError();
    }
    return go<64, 1, false, 1, false, false>(P, 1u, lds_bytes, st);
}

}  // namespace wfa
