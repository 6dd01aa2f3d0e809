// Stand-alone check of wfa_amd/csrc/wfa_altext_pk.hpp (host only): the one decoding rule behind wfa_altext_pk_write_kernel and
// wfahip_alignment_text_packed.  Every length 1 .. 70, forward and flagged: the sequence is packed into a heap block of EXACTLY
// wfahip_packed_words(len) words -- a word read outside it is an AddressSanitizer finding --, the bits of the last data word beyond
// the last base and the pad word are filled with random bits, twice, and at every start position the four-letter function and the
// base-by-base function must give the letters of a naive decode of the naive reverse complement, both times.  Then whole pairs:
// alt_pk_rows_write against wfa_altext.hpp's alt_rows_write over the corresponding bytes, and the window check at its bounds.
// Built plain and under the host sanitizers by tests/test_altext_packed_abi.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../wfa_amd/csrc/wfa_altext_pk.hpp"

#define CHECK(cond)                                                                                \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            std::fprintf(stderr, "%s:%d: %s  (len %u, rc %d, p %u)\n", __FILE__, __LINE__, #cond, len, rc, p); \
            return 1;                                                                              \
        }                                                                                          \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static uint64_t op(char letter, uint32_t count) { return ((uint64_t)(uint8_t)letter << 32) | count; }

static std::string random_acgt(uint32_t n) {
    std::string s(n, 'A');
    for (char &c : s) c = "ACGT"[rnd() & 3u];
    return s;
}

static std::string revcomp(const std::string &s) {
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : 'C';
    return r;
}

// the bases of s as a heap block of exactly alt_pk_words(len) words, tail bits and pad word random
static uint32_t *pack_exact(const std::string &s) {
    const uint32_t len = (uint32_t)s.size();
    const size_t   nw  = (size_t)wfa::alt_pk_words(len);
    uint32_t      *w   = static_cast<uint32_t *>(std::malloc(nw * 4));
    if (!w) return nullptr;
    for (size_t k = 0; k < nw; k++) w[k] = rnd();  // (the data bits are replaced below)
    for (uint32_t b = 0; b < len; b++) {
        const uint32_t code = ((uint32_t)(uint8_t)s[b] >> 1) & 3u, sh = 2u * (b & 15u);
        w[b >> 4]           = (w[b >> 4] & ~(3u << sh)) | (code << sh);
    }
    return w;
}

int main() {
    using namespace wfa;
    uint32_t len = 0, p = 0;
    int      rc = 0;
    CHECK(alt_pk_words(0) == 1 && alt_pk_words(1) == 2 && alt_pk_words(16) == 2 && alt_pk_words(17) == 3 && alt_pk_words(4294967295u) == 268435457ull);
    CHECK(alt_pk_letters_of(0xE4u) == 0x47544341u && alt_pk_letters_of(0x1Bu) == 0x41435447u && alt_pk_bswap(0x01020304u) == 0x04030201u);
    CHECK(alt_pk_funnel(0x89ABCDEFu, 0x01234567u, 0) == 0x89ABCDEFu && alt_pk_funnel(0x89ABCDEFu, 0x01234567u, 28) == 0x12345678u);
    for (len = 1; len <= 70; len++)
        for (int round = 0; round < 3; round++) {
            const std::string fwd = random_acgt(len), rev = revcomp(fwd);
            for (int fill = 0; fill < 2; fill++) {  // two fillings of the tail bits and the pad word: the same letters
                uint32_t *const w = pack_exact(fwd);
                if (!w) return 2;
                for (rc = 0; rc < 2; rc++) {
                    const std::string &want = rc ? rev : fwd;
                    for (p = 0; p < len; p++) {
                        CHECK(alt_pk_letter(w, len, rc != 0, p) == (uint8_t)want[p]);
                        if (p + 4u <= len) {
                            uint32_t v;
                            std::memcpy(&v, want.data() + p, 4);  // (base p in the low byte, as the rows are stored)
                            CHECK(alt_pk_letters4(w, len, rc != 0, p) == v);
                        }
                    }
                }
                std::free(w);
            }
        }
    // the window check: the sequence's words against n_words, then alt_window_1's trim checks, in bases of the sequence
    len = 0, rc = 0, p = 0;
    {
        uint64_t at;
        uint32_t n;
        CHECK(alt_pk_window_1(false, 10, 7, 17, 0, -5, &at, &n) && at == 0 && n == 17);   // 7 + 3 words == 10
        CHECK(!alt_pk_window_1(false, 9, 7, 17, 1, 1, &at, &n));                           // one word beyond
        CHECK(alt_pk_window_1(false, 10, 7, 32, 1, 1, &at, &n) && !alt_pk_window_1(false, 10, 7, 33, 1, 1, &at, &n));
        CHECK(alt_pk_window_1(false, 10, 9, 0, 1, 1, &at, &n) && !alt_pk_window_1(false, 10, 10, 0, 1, 1, &at, &n));  // (the pad word counts)
        CHECK(!alt_pk_window_1(false, 10, 11, 0, 1, 1, &at, &n) && !alt_pk_window_1(false, 10, ~0ull, 1, 1, 1, &at, &n));
        CHECK(!alt_pk_window_1(false, 10, (1ull << 63) + 7, 17, 1, 1, &at, &n));
        CHECK(!alt_pk_window_1(false, 1ull << 27, 0, 4294967295u, 1, 1, &at, &n) && alt_pk_window_1(false, 268435457ull, 0, 4294967295u, 1, 1, &at, &n));
        CHECK(alt_pk_window_1(true, 10, 7, 17, 3, 17, &at, &n) && at == 2 && n == 15);
        CHECK(alt_pk_window_1(true, 10, 7, 17, 18, 17, &at, &n) && at == 17 && n == 0);
        CHECK(!alt_pk_window_1(true, 10, 7, 17, 0, 17, &at, &n) && !alt_pk_window_1(true, 10, 7, 17, 1, 18, &at, &n));
        CHECK(!alt_pk_window_1(true, 10, 7, 17, 5, 3, &at, &n) && !alt_pk_window_1(true, 10, 7, 17, 1, -1, &at, &n));
        CHECK(!alt_pk_window_1(true, 10, 7, 17, -2147483647 - 1, 17, &at, &n) && !alt_pk_window_1(true, 9, 7, 17, 3, 17, &at, &n));
        AltWindow w;
        CHECK(alt_pk_window(true, 10, 0, 40, 4, 70, 3, 20, 1, 70, &w) && w.q_at == 2 && w.q_n == 18 && w.t_at == 0 && w.t_n == 70);
        CHECK(!alt_pk_window(true, 10, 0, 40, 4, 81, 3, 20, 1, 70, &w) && !alt_pk_window(true, 10, 0, 40, 4, 70, 3, 41, 1, 70, &w));
    }
    // whole pairs: ops of counts 1 .. 9 (groups of four that cross op boundaries), windows that start at every residue mod 16, both
    // strands -- the rows of exactly their length, against alt_rows_write over the bytes the words stand for
    for (int pair = 0; pair < 400; pair++) {
        std::vector<uint64_t> ops;
        const uint32_t        n_ops = 1u + rnd() % 12u;
        for (uint32_t k = 0; k < n_ops; k++) ops.push_back(op("MXIDH~"[rnd() % 6u], rnd() % 10u));
        if (pair % 7 == 0) ops.push_back(op('M', 60u + rnd() % 40u));
        const AltSums     s    = alt_sums(ops.data(), (uint32_t)ops.size());
        const uint32_t    q_at = rnd() % 20u, t_at = rnd() % 20u;
        const std::string q = random_acgt(q_at + (uint32_t)s.q + rnd() % 3u), t = random_acgt(t_at + (uint32_t)s.t + rnd() % 3u);
        len = (uint32_t)q.size(), p = (uint32_t)pair;
        for (rc = 0; rc < 2; rc++) {
            uint32_t *const qw = pack_exact(rc ? revcomp(q) : q), *const tw = pack_exact(t);  // a flagged query is stored as its reverse complement's reverse complement
            uint8_t        *rows[6];
            for (uint8_t *&r : rows) r = static_cast<uint8_t *>(std::malloc(s.cols ? (size_t)s.cols : 1));
            if (!qw || !tw || !rows[0] || !rows[1] || !rows[2] || !rows[3] || !rows[4] || !rows[5]) return 2;
            CHECK(alt_pk_rows_write(ops.data(), (uint32_t)ops.size(), qw, (uint32_t)q.size(), rc != 0, q_at, tw, (uint32_t)t.size(), t_at, rows[0],
                                    rows[1], rows[2]) == s.cols);
            CHECK(alt_rows_write(ops.data(), (uint32_t)ops.size(), reinterpret_cast<const uint8_t *>(q.data()) + q_at,
                                 reinterpret_cast<const uint8_t *>(t.data()) + t_at, rows[3], rows[4], rows[5]) == s.cols);
            for (int k = 0; k < 3; k++) CHECK(std::memcmp(rows[k], rows[k + 3], (size_t)s.cols) == 0);
            for (uint8_t *r : rows) std::free(r);
            std::free(qw), std::free(tw);
        }
    }
    std::printf("altext packed host test ok\n");
    return 0;
}
