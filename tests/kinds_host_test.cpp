// Stand-alone check of wfa_amd/csrc/wfa_kinds.hpp (host only): the kernel numbering against the literal numbers it must keep
// (they are ABI: bench.py and the tests index by them), the traits of the sub-wave forward kinds against the expressions the
// router used to derive them from, written out as literals, and bound_row_pitch() (wfa_bound.hpp) against the switch it was.
// Built under the host sanitizers by tests/test_kinds_host.py.
#include <cstdio>
#include "../wfa_amd/csrc/wfa_bound.hpp"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "%s:%d: %s  (kind %d)\n", __FILE__, __LINE__, #cond, k); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

int main() {
    using namespace wfa;
    int k = -1;
    // the numbering
    const int names[25] = {K_GENERIC, K_PACKED, K_REG,    K_BLK16,  K_BLK8,   K_BLK64,   K_NARROW, K_TEAM,  K_DUO,
                           K_BLK32,   K_LANE,   K_LONG16, K_LONG32, K_LONG64, K_LONE64,  K_LONE128, K_PAIR, K_TEAMC,
                           K_WIDE,    K_SCORE,  K_SCORE_WIDE, K_MATRIX, K_MATRIX_WIDE, K_SCORE_LONG, K_MATRIX_LONG};
    for (k = 0; k < 25; k++) CHECK(names[k] == k);
    static_assert(BLK_BATCH == 8, "the batched instances of wfa_fwd_shape.inc are compiled for eight entries per refill");

    // kinds 1 .. 15: {base, pairs per wave, row pitch, floor of a slot's words, factor on the rows, sequence windows}; 0 where the
    // router never read the value (the directory arenas have no floor and no factor, kind 7 is no sub-wave kind)
    const struct {
        int      base, pairs_wave;
        unsigned pitch, words_min, rows_mult, windows;
    } want[16] = {
        {0, 0, 0, 0, 0, 0},
        {1, 2, 0, 0, 0, 0},
        {2, 4, 0, 0, 0, 0},
        {3, 4, 64, 2048, 2, 0},
        {4, 8, 64, 2048, 2, 0},
        {5, 1, 256, 8192, 16, 0},
        {6, 8, 32, 2048, 2, 0},
        {0, 0, 0, 0, 0, 0},
        {8, 8, 32, 1024, 1, 0},
        {9, 2, 128, 4096, 4, 0},
        {10, 64, 16, 1024, 1, 0},
        {3, 4, 64, 2048, 2, 4},
        {9, 2, 128, 4096, 4, 2},
        {5, 1, 256, 8192, 16, 1},
        {3, 1, 64, 2048, 2, 1},
        {9, 1, 128, 4096, 4, 1},
    };
    for (k = 1; k <= 15; k++) {
        const KindTraits &t = kind_traits(k);
        CHECK(t.base == want[k].base);
        CHECK(t.pairs_wave == want[k].pairs_wave);
        CHECK(t.pitch == want[k].pitch);
        CHECK(t.words_min == want[k].words_min);
        CHECK(t.rows_mult == want[k].rows_mult);
        CHECK(t.windows == want[k].windows);
        // a sliding-window kind keeps a window per pair of the wave, and a base kind is its own base
        if (t.windows) CHECK(t.windows == t.pairs_wave);
        if (t.base) CHECK(kind_traits(t.base).base == t.base && kind_traits(t.base).pitch == t.pitch && kind_traits(t.base).rows_mult == t.rows_mult);
    }
    // numbers outside the table: the empty entry
    for (k = -2; k <= 40; k++)
        if (k <= 0 || k == 7 || k >= 16) CHECK(kind_traits(k).base == 0 && kind_traits(k).pitch == 0 && kind_traits(k).pairs_wave == 0);

    // bound_row_pitch(k), k = 0 .. 24: the switch it was
    const unsigned pitch_was[25] = {0, 0, 0, 64, 64, 256, 32, 0, 32, 128, 16, 64, 128, 256, 64, 128, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (k = 0; k < 25; k++) CHECK(bound_row_pitch(k) == pitch_was[k]);
    k = -1;
    CHECK(bound_row_pitch(-1) == 0 && bound_row_pitch(25) == 0 && bound_row_pitch(1 << 30) == 0);
    std::printf("kinds host test ok\n");
    return 0;
}
