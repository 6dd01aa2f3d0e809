// Stand-alone check of wfa_amd/csrc/wfa_bound.hpp (host only): the arena slot a score bound leaves a sub-wave pass, over every row
// pitch the kernels use, g = 1 .. 3 and max_score = 1 .. 4 000, against sizes the router produces (multiples of 512 words, at
// least the kind's minimum).  Built under the host sanitizers by tests/test_bounded_host.py.
#include <cstdio>
#include <cstdlib>
#include "../wfa_amd/csrc/wfa_bound.hpp"

#define CHECK(cond)                                                                                                     \
    do {                                                                                                                \
        if (!(cond)) {                                                                                                  \
            std::fprintf(stderr, "%s:%d: %s  (pitch %u g %u max_score %u words %llu)\n", __FILE__, __LINE__, #cond, pitch, g, ms, \
                         (unsigned long long)free_words);                                                               \
            return 1;                                                                                                   \
        }                                                                                                               \
    } while (0)

int main() {
    using namespace wfa;
    const uint32_t pitches[] = {16, 32, 64, 128, 256};
    // what a pass takes without a bound: the minimums of the router and sizes of short, 300-base, 1 kbp and long reads, with the rows scaled up
    const uint64_t sizes[] = {1024, 2048, 4096, 8192, 2560, 5120, 8192 + 512, 16384, 32768, 65536, 131072, 1u << 20, 1u << 24};
    unsigned long long n = 0;
    for (uint32_t pitch : pitches)
        for (uint32_t g = 1; g <= 3; g++)
            for (uint32_t ms = 1; ms <= 4000; ms++)
                for (uint64_t free_words : sizes) {
                    const uint64_t min_words = pitch == 256 ? 8192 : pitch == 128 ? 4096 : pitch <= 32 ? 1024 : 2048;
                    if (free_words < min_words) continue;
                    const uint64_t rows = bound_rows(ms, g);
                    CHECK(rows >= (uint64_t)ms / g + 1 && rows <= (uint64_t)ms / g + 2 && (rows - 1) * g >= ms);
                    const uint64_t w = bound_cap_words(free_words, pitch, min_words, ms, g);
                    CHECK(w <= free_words);                      // never more than without a bound
                    CHECK(w >= min_words && w % 512 == 0);       // the router's rounding and minimums
                    if (free_words / pitch >= (uint64_t)ms / g + 1) CHECK(w / pitch >= (uint64_t)ms / g + 1);  // the rows of the bound are there whenever they were
                    if (w < free_words) CHECK(w / pitch >= rows);  // ... and always when the bound made the slot smaller
                    const bool cov = bound_covers(w, pitch, ms, g);
                    CHECK(cov == ((w / pitch - 1) * (uint64_t)g >= ms));
                    if (w < free_words) CHECK(cov);              // a capped slot makes "out of rows" final
                    // a pair that ran out of rows computed rows 0 .. w / pitch - 1: its score is at least (w / pitch) * g
                    if (cov) CHECK((w / pitch) * (uint64_t)g > ms);
                    CHECK(bound_cap_words(free_words, pitch, min_words, 0, g) == free_words);  // no bound: untouched
                    CHECK(!bound_covers(free_words, pitch, 0, g));
                    CHECK(bound_cap_words(free_words, 0, min_words, ms, g) == free_words);     // a kind without fixed-pitch rows
                    CHECK(!bound_covers(free_words, 0, ms, g));
                    n++;
                }
    {
        const uint32_t pitch = 0, g = 0, ms = 0;
        const uint64_t free_words = 0;
        // the kinds and their pitch (wfa_fwd.hpp's numbering); directory arenas have none
        CHECK(bound_row_pitch(1) == 0 && bound_row_pitch(2) == 0 && bound_row_pitch(7) == 0 && bound_row_pitch(18) == 0);
        CHECK(bound_row_pitch(10) == 16 && bound_row_pitch(8) == 32 && bound_row_pitch(6) == 32);
        CHECK(bound_row_pitch(3) == 64 && bound_row_pitch(4) == 64 && bound_row_pitch(11) == 64 && bound_row_pitch(14) == 64);
        CHECK(bound_row_pitch(9) == 128 && bound_row_pitch(12) == 128 && bound_row_pitch(15) == 128);
        CHECK(bound_row_pitch(5) == 256 && bound_row_pitch(13) == 256);
        // the largest bound: no overflow, nothing capped that was not larger
        CHECK(bound_cap_words(1u << 20, 64, 2048, 0xFFFFFFFFu, 1) == (1u << 20));
        CHECK(bound_covers(~0ull / 2, 16, 0xFFFFFFFFu, 1));
    }
    std::printf("bounded host test ok: %llu combinations\n", n);
    return 0;
}
