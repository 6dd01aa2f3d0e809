// wfa_kinds.hpp -- the numbering of the kernels (wfahip_timing::main_kernel_kind, the `kind` of the launchers and of the router's
// passes) and what the router needs to know about a sub-wave forward kind to size its pass.  Host only, no HIP includes:
// tests/kinds_host_test.cpp compiles it stand-alone.  This is the only legend of the numbers; they are ABI (bench.py names the
// dominant kernel by them, the tests assert them) and never change.
#pragma once
#include <cstdint>

namespace wfa {

enum Kind : int {
    K_GENERIC      = 0,   // wfa_generic_kernel: a workgroup per pair, the long-pair ladder
    K_PACKED       = 1,   // wfa_packed_kernel: LDS rings of any penalty shape, two pairs per wave, directory arena
    K_REG          = 2,   // wfa_reg_kernel<2, 4, 1>: register window, four pairs per wave, directory arena
    K_BLK16        = 3,   // wfa_blk_kernel<16>: four pairs per wave, 64 diagonals
    K_BLK8         = 4,   // wfa_blk_kernel<8>: eight pairs per wave, eight diagonals per lane (option blk = 8)
    K_BLK64        = 5,   // wfa_blk_kernel<64>: a wave per pair, 256 diagonals
    K_NARROW       = 6,   // wfa_blk_kernel<8, 8, false, 4>: eight pairs per wave, 32 diagonals (short reads)
    K_TEAM         = 7,   // wfa_team_kernel: a team of workgroups per pair
    K_DUO          = 8,   // wfa_duo_kernel: 8 or 16 lanes per pair
    K_BLK32        = 9,   // wfa_blk_kernel<32>: two pairs per wave, 128 diagonals
    K_LANE         = 10,  // wfa_lane_kernel: a lane per pair (short reads)
    K_LONG16       = 11,  // K_BLK16 / K_BLK32 / K_BLK64 with sliding sequence windows: reads of any length
    K_LONG32       = 12,
    K_LONG64       = 13,
    K_LONE64       = 14,  // sliding windows, the whole wave on one pair: one / two diagonals per lane (64 / 128 diagonals)
    K_LONE128      = 15,
    K_PAIR         = 16,  // wfa_blk_kernel<64, 1, false, 1, false, false>: wfahip_align_pair, forward pass and backtrace in one launch
    K_TEAMC        = 17,  // wfa_teamc_kernel: a team of workgroups per pair, one backtrace word per diagonal
    K_WIDE         = 18,  // wfa_wide_kernel: semi-global reads up to 2 047 bases, the rows in 16-bit LDS rings
    K_SCORE        = 19,  // wfa_score_kernel (wfahip_score_batch, global pairs)
    K_SCORE_WIDE   = 20,  // wfa_wide_kernel<.., SCORE> (wfahip_score_batch, semi-global pairs)
    K_MATRIX       = 21,  // wfa_score_kernel<MATRIX> (wfahip_score_matrix, global alignment)
    K_MATRIX_WIDE  = 22,  // wfa_wide_kernel<.., SCORE, MATRIX> (wfahip_score_matrix, semi-global alignment)
    K_SCORE_LONG   = 23,  // wfa_score_long_kernel (wfahip_score_batch: reads beyond 2 047 bases took most of the call)
    K_MATRIX_LONG  = 24   // wfa_score_long_kernel<MATRIX> (wfahip_score_matrix, likewise by cells)
};

constexpr int BLK_BATCH = 8;  // pairs a group of K_BLK16 / K_NARROW stages at a time (short reads, FWD_BATCH)

// A sub-wave forward kind as the router's pass sees it.  The arena of a slot is fixed-pitch rows -- one row of `pitch` 32-bit
// words per score index, max(round512(words_dir * rows_mult * arena_mult), words_min) words -- or, with pitch 0, a directory
// of words_dir words that no multiplier and no score bound touches.
struct KindTraits {
    uint8_t  base;        // the kind whose arena format it writes (the sliding-window kinds share their plain kind's)
    uint8_t  pairs_wave;  // pairs a wave works on
    uint16_t pitch;       // 32-bit words per arena row; 0: directory arena
    uint16_t words_min;   // floor of a slot's words
    uint8_t  rows_mult;   // factor on words_dir * arena_mult
    uint8_t  windows;     // sliding-window kinds: sequence windows a wave keeps in LDS (= pairs_wave); 0: whole sequences
};

constexpr int N_FWD_KINDS = 16;
constexpr KindTraits KIND_TRAITS[N_FWD_KINDS] = {
    {},                                 // K_GENERIC: no sub-wave pass
    {K_PACKED, 2, 0, 0, 0, 0},
    {K_REG, 4, 0, 0, 0, 0},
    {K_BLK16, 4, 64, 2048, 2, 0},
    {K_BLK8, 8, 64, 2048, 2, 0},
    {K_BLK64, 1, 256, 8192, 16, 0},
    {K_NARROW, 8, 32, 2048, 2, 0},
    {},                                 // K_TEAM
    {K_DUO, 8, 32, 1024, 1, 0},         // 64 diagonals x 16 bit
    {K_BLK32, 2, 128, 4096, 4, 0},
    {K_LANE, 64, 16, 1024, 1, 0},       // 32 diagonals x 16 bit
    {K_BLK16, 4, 64, 2048, 2, 4},
    {K_BLK32, 2, 128, 4096, 4, 2},
    {K_BLK64, 1, 256, 8192, 16, 1},
    {K_BLK16, 1, 64, 2048, 2, 1},
    {K_BLK32, 1, 128, 4096, 4, 1},
};

// (any other number: the empty entry -- no pass, no pitch)
constexpr const KindTraits &kind_traits(int kind) { return KIND_TRAITS[kind > 0 && kind < N_FWD_KINDS ? kind : 0]; }

}  // namespace wfa
