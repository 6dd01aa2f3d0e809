// Stand-alone check of wfa_amd/csrc/wfa_pile.hpp (host only): the one counting rule behind wfa_pile_kernel, wfa_pile_pk_kernel,
// wfahip_pileup and wfahip_pileup_packed.  pile_pair against a naive walk that goes column by column and tests every base against
// the window; pile_clip against brute force; pile_pk_code against the display rows' letters on both strands.  The ops, the query's
// bytes and words and the counters each sit in a heap block of EXACTLY their size -- a byte, a word or a counter touched outside one
// is an AddressSanitizer finding.  Then the seams: a 'D' run at ts == 0 and at the window's end, an empty target window, windows
// that cut an op, counts of 0xFFFFFFFF in the sums (no column outside the window may be walked: the program would not end), and
// EXTRA_BASES wrapping.  Built plain and under the host sanitizers by tests/test_pile_host.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../wfa_amd/csrc/wfa_pile.hpp"

using namespace wfa;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static uint64_t op(char letter, uint32_t count) { return ((uint64_t)(uint8_t)letter << 32) | count; }

// a heap block of exactly n elements
template <class T>
struct Exact {
    T     *p;
    size_t n;
    explicit Exact(size_t n_) : p(static_cast<T *>(std::malloc(n_ ? n_ * sizeof(T) : 1))), n(n_) { std::memset(p, 0, n_ ? n_ * sizeof(T) : 1); }
    Exact(const Exact &) = delete;
    ~Exact() { std::free(p); }
};

static uint32_t naive_word(uint8_t b) {
    switch (b) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'T': case 't': return 2;
    case 'G': case 'g': return 3;
    default: return 4;
    }
}

// the rule, column by column, every base tested against the window; q: the counter word of every base of the query's window
static void naive(const std::vector<uint64_t> &ops, const std::vector<uint32_t> &q, uint64_t T0, uint32_t t_n, uint64_t at, uint64_t n,
                  std::vector<uint32_t> &counts) {
    uint64_t   qs = 0, ts = 0;
    const auto add = [&](uint64_t P, uint32_t word, uint32_t v) {
        if (P >= at && P - at < n) counts[(size_t)(P - at) * 8 + word] += v;
    };
    for (uint64_t o : ops) {
        const char     letter = (char)(o >> 32);
        const uint32_t c      = (uint32_t)o;
        if (letter == 'M' || letter == 'X') {
            for (uint32_t x = 0; x < c; x++) add(T0 + ts + x, q[(size_t)(qs + x)], 1);
            qs += c, ts += c;
        } else if (letter == 'I') {
            for (uint32_t x = 0; x < c; x++) add(T0 + ts + x, 5, 1);
            ts += c;
        } else if (letter == 'D') {
            if (c && t_n) add(T0 + (ts ? ts : 1) - 1, 6, 1), add(T0 + (ts ? ts : 1) - 1, 7, c);
            qs += c;
        } else if (letter == 'H') {
            qs += c;
        }
    }
}

static std::vector<uint32_t> run(const std::vector<uint64_t> &ops, const PileByteSeq *bs, const PilePkSeq *ps, uint64_t T0, uint32_t t_n,
                                 uint64_t at, uint64_t n) {
    Exact<uint64_t> o(ops.size());
    if (!ops.empty()) std::memcpy(o.p, ops.data(), ops.size() * 8);
    Exact<uint32_t> c((size_t)n * 8);
    const PileWin   W   = {at, n};
    const auto      add = [&](uint64_t idx, uint32_t word, uint32_t v) { c.p[idx * PILE_WORDS + word] += v; };
    if (bs) pile_pair(o.p, (uint32_t)ops.size(), *bs, T0, t_n, W, add);
    else pile_pair(o.p, (uint32_t)ops.size(), *ps, T0, t_n, W, add);
    return std::vector<uint32_t>(c.p, c.p + (size_t)n * 8);
}

// a reader that owns no memory: the word of base p is p % 5, and the largest base asked for is kept
struct CountingSeq {
    mutable uint64_t asked = 0, max_p = 0;
    uint32_t         word(uint64_t p) const {
        asked++;
        if (p > max_p) max_p = p;
        return (uint32_t)(p % 5u);
    }
};

int main() {
    static_assert(PILE_WORDS == 8 && PILE_W_A == 0 && PILE_W_C == 1 && PILE_W_T == 2 && PILE_W_G == 3 && PILE_W_OTHER == 4 && PILE_W_GAP == 5 &&
                      PILE_W_EXTRA == 6 && PILE_W_EXTRA_BASES == 7,
                  "the words");
    // ---- the word of a byte, all 256
    for (uint32_t b = 0; b < 256; b++) CHECK(pile_word_of_byte(b) == naive_word((uint8_t)b));

    // ---- the code of a packed base is the display rows' letter, on both strands, from words in a block of exactly their size
    for (uint32_t len = 1; len <= 70; len++) {
        Exact<uint32_t> w((size_t)alt_pk_words(len));
        for (size_t k = 0; k < w.n; k++) w.p[k] = rnd();
        for (int rc = 0; rc < 2; rc++)
            for (uint32_t p = 0; p < len; p++) {
                const uint32_t code = pile_pk_code(w.p, len, rc != 0, p);
                CHECK(code < 4u && "ACTG"[code] == (char)alt_pk_letter(w.p, len, rc != 0, p));
                CHECK(pile_word_of_byte((uint8_t)"ACTG"[code]) == code);
            }
    }

    // ---- pile_clip against brute force, every small case; then far from 0
    for (uint64_t P0 = 0; P0 < 12; P0++)
        for (uint64_t n = 0; n < 9; n++)
            for (uint64_t at = 0; at < 14; at++)
                for (uint64_t wn = 0; wn < 9; wn++) {
                    uint64_t lo = 99, hi = 99, blo = n, bhi = 0;
                    for (uint64_t c = 0; c < n; c++)
                        if (P0 + c >= at && P0 + c < at + wn) {
                            if (c < blo) blo = c;
                            bhi = c + 1;
                        }
                    const bool any = pile_clip(P0, n, PileWin{at, wn}, &lo, &hi);
                    CHECK(any == (bhi != 0));
                    if (any) CHECK(lo == blo && hi == bhi);
                    uint64_t idx;
                    CHECK(pile_in(P0, PileWin{at, wn}, &idx) == (P0 >= at && P0 < at + wn));
                }
    {
        uint64_t lo, hi;
        CHECK(pile_clip(5, 0xFFFFFFFFull, PileWin{0xFFFFFFF0ull, 100}, &lo, &hi) && lo == 0xFFFFFFEBull && hi == 0xFFFFFFFFull);
        CHECK(pile_clip(1ull << 40, 64ull * 0xFFFFFFFFull, PileWin{(1ull << 40) + 7, PILE_MAX_N}, &lo, &hi) && lo == 7 && hi == 64ull * 0xFFFFFFFFull);
        CHECK(!pile_clip(10, 5, PileWin{~0ull - 3, 4}, &lo, &hi));
        CHECK(pile_clip(~0ull - 9, 5, PileWin{~0ull - 7, 8}, &lo, &hi) && lo == 2 && hi == 5);
        uint64_t idx;
        CHECK(pile_in(~0ull, PileWin{~0ull - 3, 4}, &idx) && idx == 3);
        CHECK(!pile_in(2, PileWin{~0ull - 3, 4}, &idx));
        CHECK(pile_extra_base(100, 0) == 100 && pile_extra_base(100, 1) == 100 && pile_extra_base(100, 9) == 108);
    }

    // ---- random pairs, random windows (most cut an op), from bytes and from words on both strands
    for (int iter = 0; iter < 3000; iter++) {
        const uint32_t        n_ops = rnd() % 12u;
        std::vector<uint64_t> ops;
        uint32_t              q_used = 0, t_used = 0;
        for (uint32_t k = 0; k < n_ops; k++) {
            const char     letter = "MXIDHMXID~"[rnd() % 10u];
            const uint32_t c      = rnd() % 6u == 0 ? 0u : 1u + rnd() % (iter % 7 == 0 ? 40u : 6u);
            ops.push_back(op(letter, c));
            if (letter == 'M' || letter == 'X' || letter == 'D' || letter == 'H') q_used += c;
            if (letter == 'M' || letter == 'X' || letter == 'I') t_used += c;
        }
        const uint32_t q_slack = rnd() % 3u, t_n = t_used + rnd() % 3u;
        const uint64_t T0 = 50 + rnd() % 50u, at = 40 + rnd() % 80u, wn = rnd() % 60u;
        // bytes: any byte value
        {
            Exact<uint8_t>        q(q_used + q_slack);
            std::vector<uint32_t> qw;
            for (size_t k = 0; k < q.n; k++) q.p[k] = rnd() % 3u ? (uint8_t) "ACGTacgt"[rnd() & 7u] : (uint8_t)rnd(), qw.push_back(naive_word(q.p[k]));
            std::vector<uint32_t> want((size_t)wn * 8, 0u);
            naive(ops, qw, T0, t_n, at, wn, want);
            const PileByteSeq S = {q.p};
            CHECK(run(ops, &S, nullptr, T0, t_n, at, wn) == want);
        }
        // words: the window [q_at, q_at + q_used) of a longer sequence, forward and flagged
        for (int rc = 0; rc < 2; rc++) {
            const uint32_t  q_at = rnd() % 20u, q_len = q_at + q_used + q_slack + rnd() % 20u;
            Exact<uint32_t> w((size_t)alt_pk_words(q_len));
            for (size_t k = 0; k < w.n; k++) w.p[k] = rnd();
            std::vector<uint32_t> qw;
            for (uint32_t p = 0; p < q_used + q_slack; p++) qw.push_back(naive_word(alt_pk_letter(w.p, q_len, rc != 0, q_at + p)));
            std::vector<uint32_t> want((size_t)wn * 8, 0u);
            naive(ops, qw, T0, t_n, at, wn, want);
            const PilePkSeq S = {w.p, q_len, q_at, rc != 0};
            CHECK(run(ops, nullptr, &S, T0, t_n, at, wn) == want);
        }
    }

    // ---- the seams, by hand.  Query ACGTACGT, target window of 6 bases at coordinate 100
    {
        Exact<uint8_t> q(8);
        std::memcpy(q.p, "ACGTACGT", 8);
        const PileByteSeq S = {q.p};
        // a D run at ts == 0 shares base 0's counters; one at the window's end hangs on the last base
        std::vector<uint64_t> ops = {op('D', 2), op('M', 6), op('D', 0), op('D', 3)};
        Exact<uint8_t>        q11(11);
        std::memcpy(q11.p, "ACGTACGTACG", 11);
        const PileByteSeq S11 = {q11.p};
        auto              c   = run(ops, &S11, nullptr, 100, 6, 100, 6);
        CHECK(c[0 * 8 + 6] == 1 && c[0 * 8 + 7] == 2 && c[5 * 8 + 6] == 1 && c[5 * 8 + 7] == 3);
        CHECK(c[0 * 8 + 3] == 1 && c[1 * 8 + 2] == 1 && c[2 * 8 + 0] == 1 && c[3 * 8 + 1] == 1 && c[4 * 8 + 3] == 1 && c[5 * 8 + 2] == 1);  // G T A C G T
        // ... and is outside a window that ends one base earlier, or begins one base later
        c = run(ops, &S11, nullptr, 100, 6, 100, 5);
        CHECK(c[0 * 8 + 6] == 1 && c[4 * 8 + 6] == 0 && c[4 * 8 + 7] == 0 && c[4 * 8 + 3] == 1);
        c = run(ops, &S11, nullptr, 100, 6, 101, 5);
        CHECK(c[0 * 8 + 6] == 0 && c[0 * 8 + 2] == 1 && c[4 * 8 + 6] == 1 && c[4 * 8 + 7] == 3);
        // an empty target window: D and H alone, nothing is added -- not even at the coordinate the run would hang on
        ops = {op('D', 5), op('H', 3)};
        c   = run(ops, &S, nullptr, 100, 0, 90, 20);
        for (uint32_t v : c) CHECK(v == 0);
        // the same ops over a target window of one base that no op consumes: the run hangs on it
        c = run(ops, &S, nullptr, 100, 1, 90, 20);
        CHECK(c[10 * 8 + 6] == 1 && c[10 * 8 + 7] == 5);
        // windows that cut an op: 3 of the 8 M columns, and the I op's middle
        ops = {op('M', 8), op('I', 9)};
        c   = run(ops, &S, nullptr, 100, 17, 103, 3);
        CHECK(c[0 * 8 + 2] == 1 && c[1 * 8 + 0] == 1 && c[2 * 8 + 1] == 1);  // T A C: query bases 3, 4, 5
        c = run(ops, &S, nullptr, 100, 17, 110, 4);
        CHECK(c[0 * 8 + 5] == 1 && c[3 * 8 + 5] == 1 && c[0 * 8 + 0] == 0);
        // a window before, behind and far from the pair
        for (uint64_t at : {0ull, 94ull, 117ull, 1ull << 62, ~0ull - 5}) {
            c = run(ops, &S, nullptr, 100, 17, at, 6);
            for (uint32_t v : c) CHECK(v == 0);
        }
    }
    // ---- counts of 0xFFFFFFFF: the sums are 64-bit, and only the columns inside the window are walked
    {
        const uint32_t        BIG = 0xFFFFFFFFu;
        std::vector<uint64_t> ops = {op('M', BIG), op('I', BIG), op('D', BIG), op('X', BIG), op('D', 2), op('D', BIG), op('H', BIG), op('M', 3)};
        Exact<uint64_t>       o(ops.size());
        std::memcpy(o.p, ops.data(), ops.size() * 8);
        const uint64_t  T0 = 1000, at = T0 + 3ull * BIG - 4, n = 9;  // the last 4 X columns, the 3 M columns, 2 beyond
        Exact<uint32_t> c((size_t)n * 8);
        CountingSeq     S;
        pile_pair(o.p, (uint32_t)ops.size(), S, T0, BIG, PileWin{at, n}, [&](uint64_t idx, uint32_t word, uint32_t v) { c.p[idx * 8 + word] += v; });
        CHECK(S.asked == 7 && S.max_p == 5ull * BIG + 2 + 2);  // query: M, D, X, D, H of 0xFFFFFFFF, D 2, then the last M's third base
        uint64_t total = 0;
        for (size_t k = 0; k < c.n; k++) total += c.p[k];
        // the X op's last base carries both D runs behind it: EXTRA 2, EXTRA_BASES 2 + 0xFFFFFFFF wraps to 1
        CHECK(c.p[3 * 8 + 6] == 2 && c.p[3 * 8 + 7] == 1u);
        CHECK(total == 7 + 2 + 1);
        // the first D run hangs on the last I base, far before the window; a window there sees it, and the X op's first base
        Exact<uint32_t> d(2 * 8);
        pile_pair(o.p, (uint32_t)ops.size(), S, T0, BIG, PileWin{T0 + 2ull * BIG - 1, 2},
                  [&](uint64_t idx, uint32_t word, uint32_t v) { d.p[idx * 8 + word] += v; });
        CHECK(d.p[0 * 8 + 5] == 1 && d.p[0 * 8 + 6] == 1 && d.p[0 * 8 + 7] == BIG && d.p[1 * 8 + (2ull * BIG) % 5u] == 1);
    }
    std::printf("pile host test ok\n");
    return 0;
}
