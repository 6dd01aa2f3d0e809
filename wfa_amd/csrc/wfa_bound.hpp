// wfa_bound.hpp -- the arithmetic of a score bound on the row-indexed arenas (wfahip_align_batch_bounded).  Host only, no HIP
// includes: tests/bounded_host_test.cpp compiles it stand-alone.
//
// The sub-wave forward kernels whose arena is fixed-pitch rows -- one row of `pitch` 32-bit words per score index -- stop a
// pair when its score index reaches the rows of its slot (`no_room` in wfa_duo.hpp and wfa_blk.hpp, the rows_cap test in
// wfa_lane.hpp: row si is neither computed further nor stored once si >= words / pitch) and hand it on as ST_REDO_ARENA.
// A pair handed on that way has computed the rows 0 .. words / pitch - 1 and none of them terminated: its score is above
// (words / pitch - 1) * g.  So a slot sized by the bound turns "out of rows" into "above the bound".
#pragma once
#include <algorithm>
#include <cstdint>
#include "wfa_kinds.hpp"

namespace wfa {

// 32-bit words per arena row of the sub-wave forward kernel `kind` (wfa_kinds.hpp); 0: the kind's arena is not fixed-pitch rows
// (K_PACKED and K_REG keep a directory), the bound does not size it
inline uint32_t bound_row_pitch(int kind) { return kind_traits(kind).pitch; }

// rows a slot gets under the bound: the score indices 0 .. max_score / g every score up to the bound needs, and one more when g
// does not divide max_score -- (rows - 1) * g then reaches max_score itself, which is what bound_covers asks, and a slot that
// the bound made smaller always makes "out of rows" final
inline uint64_t bound_rows(uint32_t max_score, uint32_t g) {
    const uint64_t gg = std::max<uint32_t>(g, 1);
    return ((uint64_t)max_score + gg - 1) / gg + 1;
}

// words of a slot under the bound: never more than `words` (what the pass would take without a bound: a multiple of 512, at least
// min_words), and when capped the bound's rows, rounded and floored as `words` was
inline uint64_t bound_cap_words(uint64_t words, uint32_t pitch, uint64_t min_words, uint32_t max_score, uint32_t g) {
    if (max_score == 0 || pitch == 0) return words;
    const uint64_t need = std::max<uint64_t>((bound_rows(max_score, g) * pitch + 511) & ~511ull, min_words);
    return std::min(words, need);
}

// the slot's rows reach the bound: a pair that ran out of them has a score above max_score
inline bool bound_covers(uint64_t words, uint32_t pitch, uint32_t max_score, uint32_t g) {
    if (max_score == 0 || pitch == 0) return false;
    const uint64_t rows = words / pitch;
    return rows >= 1 && (rows - 1) * std::max<uint32_t>(g, 1) >= max_score;
}

}  // namespace wfa
