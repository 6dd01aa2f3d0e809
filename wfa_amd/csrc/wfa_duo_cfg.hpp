// wfa_duo_cfg.hpp -- sizes of wfa_duo_kernel (wfa_duo.hpp) that the host needs too, and its launcher.
// The kernel lives in a translation unit of its own (wfa_duo.hip) because it is compiled with
// -mllvm -amdgpu-atomic-optimizer-strategy=None: its prefetch claims queue entries with an atomicAdd whose result must
// NOT be waited for on the spot, and LLVM's atomic optimizer turns a uniform atomicAdd into a wave-aggregated atomic
// followed at once by s_waitcnt + v_readfirstlane.  The other kernels want the optimizer: the lane-per-pair backtrace
// reserves its CIGAR op slots with one atomicAdd per lane, which the optimizer folds into one per wave (with the flag on
// the whole library that kernel went from 1.2 to 19 ms).
#pragma once
#include "wfa_common.hpp"

namespace wfa {

#ifndef WFA_DUO_WAVES
#define WFA_DUO_WAVES 4  // waves per SIMD the kernel is compiled for
#endif
#ifndef WFA_DUO_PARK
#define WFA_DUO_PARK 4
#endif
#ifndef WFA_DUO_WIDEN_AT
#define WFA_DUO_WIDEN_AT 26
#endif
#ifndef WFA_DUO_NARROW_AT
#define WFA_DUO_NARROW_AT 21
#endif
#ifndef WFA_DUO_GROUP_MAJOR
#define WFA_DUO_GROUP_MAJOR 2
#endif
// WF_EXTEND of the score step (wfa_duo.hpp): 1 = candidates as lane masks, continuation 32 bases a round (the default);
// 0 = the form before it (cmask in a register, 16 bases a round), kept for A/B builds: scripts/mkvariant.sh <name> -DWFA_DUO_EXTEND=0
#ifndef WFA_DUO_EXTEND
#define WFA_DUO_EXTEND 1
#endif
// Queue claims of the prefetch (wfa_duo.hpp): the most fetches a wave claims with one atomic on the queue's head word, 1 .. 8.  Above 1 a wave
// also starts with eight entries of its own, no atomic; 1 = one fetch per atomic from entry 0 on (the claiming before blocks), kept for A/B
// builds -- scripts/mkvariant.sh <name> -DWFA_DUO_CLAIM=1 -- and, as debug option duo_claim, for the tests.  4 measured best: 1e6 x 1 kbp at
// 4/6/2 14.33 ms a step against 14.35 with 2 and 14.46 with 8, at 2/4/2 9.13 against 9.25 and 9.18 (profiles/r09_duo_claim.txt)
#ifndef WFA_DUO_CLAIM
#define WFA_DUO_CLAIM 4
#endif
// Where a freed half row takes its next pair (wfa_duo.hpp): 1 = in the finish branch of the score step that freed it (the default; a
// restructuring round only places what that could not); 0 = always in a restructuring round, the form before, kept for A/B builds:
// scripts/mkvariant.sh <name> -DWFA_DUO_FILL=0
#ifndef WFA_DUO_FILL
#define WFA_DUO_FILL 1
#endif
// How the score step asks wave-uniform questions and where it keeps what only set_derived() changes (wfa_duo.hpp): 1 = "does any lane ..." is a
// scalar compare of the lane mask the vector compare wrote, the masks of the running and of the wide lanes live in scalar registers, and the
// lane's diagonal indices and its trigger edge are formed once per set_derived() (the default); 0 = the form before -- every such test through a
// 0/1 vector register, the constants formed in every step -- kept for A/B builds: scripts/mkvariant.sh <name> -DWFA_DUO_UNIFORM=0
// (wfa_duo_kernel only: the 32-bit-ring reference wfa_duo32_kernel keeps the form before either way -- profiles/r13_duo_uniform.txt)
#ifndef WFA_DUO_UNIFORM
#define WFA_DUO_UNIFORM 1
#endif
// Where the score step keeps its wave-uniform state and the kernel its cold arguments (wfa_duo.hpp): 1 = the arguments that only cold code reads
// (arena, pair_meta, the redo list, work, chunk_first, queue_head, chunk_n, prepack, g, census) are loaded from the kernel-argument segment where
// they are used and hold no scalar register while the steps run; the prefetch's flags and buffer masks are said to be uniform where they are
// written, not at the head of every step; `slow` has a lane mask like `run` and `wide`; the row store's "has the lane a cell" is the OR of the four
// cell masks; the score index moves on with one add-with-carry (the default).  0 = the form before, kept for A/B builds:
// scripts/mkvariant.sh <name> -DWFA_DUO_SCALAR=0.  (wfa_duo_kernel in its WFA_DUO_UNIFORM form only -- profiles/r15_duo_scalar.txt)
#ifndef WFA_DUO_SCALAR
#define WFA_DUO_SCALAR 1
#endif
// ... and which of its five items, one bit each, for A/B builds of a single item: 1 the reloaded arguments, 2 the uniform state, 4 slow_m, 8 the
// store's test from the cell masks, 16 the add-with-carry (31 = all, the default; vector instructions each takes off a step: 0, 3, 2, 3, 1)
#ifndef WFA_DUO_SCALAR_ITEMS
#define WFA_DUO_SCALAR_ITEMS 31
#endif
// Arena layout of wfa_duo_kernel (16-bit words; a lane's four diagonals of a score are one 8-byte store, and 8 scores of them
// one 64-byte piece, in every one of the three):
//   0  CompactView fmt 7 (round 3) -- tiles of 8 scores x 64 diagonals (1 KB), inside a tile [diagonal / 4][score & 7][diagonal & 3]:
//      the row pointer needs "next score, and the next tile after every eighth" -- seven vector instructions a step;
//   1  fmt 9 (round 6) -- group-major, [diagonal / 4 & 15][score][diagonal & 3]: a constant stride, and the backtrace's walk,
//      which stays within a few groups, reads from a handful of DRAM pages instead of one per tile.  But ONE lane fills a
//      128-byte line, over 16 steps: twice the dirty lines in L2, evicted half-written and written again -- WRITE_SIZE 26 GB
//      per 1e6 x 1 kbp pairs instead of 10.8;
//   2  fmt 10 (round 6, the default) -- the groups two by two: [diagonal / 8 & 7][score / 8][diagonal / 4 & 1][score & 7][diagonal & 3].
//      A 128-byte line is filled by two neighbouring lanes in 8 steps as in the tiles, a pair of groups is contiguous over
//      all the scores as in fmt 9, and the address comes from the score index (and, add, shift-add) with no pointer to carry.
constexpr uint32_t DUO_ARENA_FMT = WFA_DUO_GROUP_MAJOR == 2 ? 10u : WFA_DUO_GROUP_MAJOR == 1 ? 9u : 7u;
constexpr int DUO_PARK       = WFA_DUO_PARK;           // park records per wave
constexpr int DUO_PARK_WORDS = 8 * 12 + 16;            // rings of 8 lanes, two 16-bit offsets per word (reads under 2 048 bases) + 16 scalars
constexpr int DUO_BUFS       = 8 + 1 + DUO_PARK;       // sequence buffers per wave: running pairs, staging, parked pairs (one pair per fetch)
constexpr int DUO_FETCH_MAX  = 8;                      // short reads: pairs per fetch (as many prepacked slots as one 16-byte load per lane covers)
constexpr int DUO_WIDEN_AT   = WFA_DUO_WIDEN_AT;       // a narrow pair whose band spans more diagonals than this widens (a recentred band must fit 32 - 6)
constexpr int DUO_NARROW_AT  = WFA_DUO_NARROW_AT;      // a wide pair whose band spans at most this many narrows
constexpr int DUO_WIDE_MAX   = 56;                     // a wide pair whose band spans more is handed on
constexpr int DUO_CLAIM_MAX  = 8;                      // most fetches per queue claim (KParams::duo_claim, 1 .. DUO_CLAIM_MAX)
constexpr int DUO_CLAIM      = WFA_DUO_CLAIM;          // ... and the default
static_assert(DUO_CLAIM >= 1 && DUO_CLAIM <= DUO_CLAIM_MAX, "WFA_DUO_CLAIM: 1 .. 8 fetches per claim");

// pairs one fetch brings in: the slots of consecutive queue entries are contiguous in the prepack buffer, and one
// 16-byte load per lane covers 256 words -- eight slots of a 150-base pair, one of a 1 kbp pair
__host__ __device__ inline uint32_t duo_fetch_pairs(uint32_t prepack_words) {
    const uint32_t f = 256u / prepack_words;
    return f < 1u ? 1u : (f > (uint32_t)DUO_FETCH_MAX ? (uint32_t)DUO_FETCH_MAX : f);
}
__host__ __device__ inline uint32_t duo_bufs(uint32_t prepack_words) { return 8u + duo_fetch_pairs(prepack_words) + (uint32_t)DUO_PARK; }
__host__ __device__ inline uint32_t duo_lds_words(uint32_t prepack_words) {
    return duo_bufs(prepack_words) * prepack_words + (uint32_t)DUO_PARK * DUO_PARK_WORDS;
}

// launches wfa_duo_kernel<census, DX, DOE> of penalty shape `shape` (wfa_duo.hip; wfa_fwd.hpp: fwd_shape()) -- or, pk = false, its
// 32-bit-ring reference wfa_duo32_kernel (debug option duo_pk = 0)
hipError_t wfa_launch_duo(int shape, const KParams &P, uint32_t grid, size_t lds_bytes, hipStream_t st, bool census, bool pk);

}  // namespace wfa
