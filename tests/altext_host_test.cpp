// Stand-alone check of wfa_amd/csrc/wfa_altext.hpp (host only): the one rendering rule behind the display-row kernels and
// wfahip_alignment_text.  Every pair is rendered from heap copies of EXACTLY its ops and EXACTLY its windows' bytes into heap rows
// of EXACTLY the computed length, so that a byte read past a window or written past a row is an AddressSanitizer finding; the rows
// are compared with a column-by-column restatement.  Built plain and under the host sanitizers by tests/test_altext_abi.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../wfa_amd/csrc/wfa_altext.hpp"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "%s:%d: %s  (case %d)\n", __FILE__, __LINE__, #cond, which); \
            return 1;                                                            \
        }                                                                        \
    } while (0)

static uint64_t op(char letter, uint32_t count) { return ((uint64_t)(uint8_t)letter << 32) | count; }

template <class T>
static T *heap_copy(const T *src, size_t n) {  // exactly n elements (one byte when n == 0, never dereferenced)
    T *p = static_cast<T *>(std::malloc(n ? n * sizeof(T) : 1));
    if (p && n) std::memcpy(p, src, n * sizeof(T));
    return p;
}

struct Pair {
    std::vector<uint64_t> ops;
    std::string           q, t;
    int32_t               qbegin, qend, tbegin, tend;
};

// the restatement: the reference's loop, one column at a time
static void naive(const Pair &p, bool trim, std::string rows[3]) {
    size_t a = 0, b = p.ops.size();
    std::string q = p.q, t = p.t;
    if (trim) {
        while (a < b && (p.ops[a] >> 32) != 'M') a++;
        while (b > a && (p.ops[b - 1] >> 32) != 'M') b--;
        if (a == b) return;
        q = p.q.substr((size_t)(p.qbegin - 1), (size_t)(p.qend - p.qbegin + 1));
        t = p.t.substr((size_t)(p.tbegin - 1), (size_t)(p.tend - p.tbegin + 1));
    }
    size_t v = 0, h = 0;
    for (size_t k = a; k < b; k++) {
        const char     l = (char)(p.ops[k] >> 32);
        const uint32_t n = (uint32_t)p.ops[k];
        for (uint32_t x = 0; x < n; x++) {
            if (l == 'M' || l == 'X') rows[0] += q.at(v++), rows[1] += l == 'M' ? '|' : ' ', rows[2] += t.at(h++);
            else if (l == 'I') rows[0] += '-', rows[1] += ' ', rows[2] += t.at(h++);
            else if (l == 'D' || l == 'H') rows[0] += q.at(v++), rows[1] += ' ', rows[2] += '-';
        }
    }
}

int main() {
    using namespace wfa;
    int which = 0;
    // one op at a time
    CHECK(alt_kind(op('M', 3)) == (ALT_Q | ALT_T) && alt_kind(op('X', 3)) == (ALT_Q | ALT_T) && alt_kind(op('I', 3)) == ALT_T);
    CHECK(alt_kind(op('D', 3)) == ALT_Q && alt_kind(op('H', 3)) == ALT_Q && alt_kind(op('~', 3)) == 0u && alt_kind(op('m', 3)) == 0u);
    CHECK(alt_kind(((uint64_t)0x100 + 'M') << 32 | 3u) == 0u);  // the letter is the whole upper word
    CHECK(alt_cols(op('M', 4294967295u)) == 4294967295u && alt_cols(op('~', 7)) == 0u && alt_cols(op('I', 0)) == 0u);
    CHECK(alt_a_byte(op('M', 1)) == '|' && alt_a_byte(op('X', 1)) == ' ' && alt_a_byte(op('I', 1)) == ' ' && alt_a_byte(op('D', 1)) == ' ');
    {  // 64-bit sums: 64 ops of a full u32
        std::vector<uint64_t> big(64, op('M', 4294967295u));
        const AltSums         s = alt_sums(big.data(), 64);
        CHECK(s.cols == 64ull * 4294967295ull && s.q == s.cols && s.t == s.cols);
    }
    // the windows
    which = 100;
    {
        AltWindow w;
        CHECK(alt_window(false, 100, 10, 20, 40, 60, 0, -7, 99, 0, &w) && w.q_at == 10 && w.q_n == 20 && w.t_at == 40 && w.t_n == 60);
        CHECK(!alt_window(false, 100, 10, 20, 40, 61, 1, 1, 1, 1, &w));                  // the target leaves the blob by one byte
        CHECK(!alt_window(false, 100, 81, 20, 40, 60, 1, 1, 1, 1, &w));
        CHECK(!alt_window(false, 100, ~0ull, 2, 40, 60, 1, 1, 1, 1, &w) && !alt_window(false, 100, 101, 0, 40, 60, 1, 1, 1, 1, &w));
        CHECK(alt_window(false, 100, 100, 0, 40, 60, 1, 1, 1, 1, &w));                   // an empty sequence at the very end is inside
        CHECK(alt_window(true, 100, 10, 20, 40, 60, 3, 20, 1, 60, &w) && w.q_at == 12 && w.q_n == 18 && w.t_at == 40 && w.t_n == 60);
        CHECK(alt_window(true, 100, 10, 20, 40, 60, 21, 20, 5, 4, &w) && w.q_n == 0 && w.t_n == 0 && w.q_at == 30 && w.t_at == 44);
        CHECK(!alt_window(true, 100, 10, 20, 40, 60, 0, 20, 1, 60, &w));                 // BEGIN = 0
        CHECK(!alt_window(true, 100, 10, 20, 40, 60, -2147483647 - 1, 20, 1, 60, &w));
        CHECK(!alt_window(true, 100, 10, 20, 40, 60, 1, 21, 1, 60, &w));                 // END = len + 1
        CHECK(!alt_window(true, 100, 10, 20, 40, 60, 1, 20, 1, 61, &w));
        CHECK(!alt_window(true, 100, 10, 20, 40, 60, 5, 3, 1, 60, &w));                  // BEGIN - 1 > END
        CHECK(!alt_window(true, 100, 10, 20, 40, 60, 1, 20, 2, 0, &w));
        CHECK(!alt_window(true, 100, 10, 20, 40, 60, 1, -1, 1, 60, &w));
        CHECK(alt_window(true, 1ull << 40, 10, 4294967295u, 40, 60, 2147483647, 2147483647, 1, 60, &w) && w.q_n == 1);
        const AltSums fit = {30, 18, 60}, q1 = {30, 19, 60}, t1 = {30, 18, 61};
        CHECK(alt_window(true, 100, 10, 20, 40, 60, 3, 20, 1, 60, &w) && alt_fits(fit, w) && !alt_fits(q1, w) && !alt_fits(t1, w));
    }
    // whole pairs, both modes
    std::vector<Pair> pairs;
    pairs.push_back({{op('M', 10)}, "ACGTACGTAC", "ACGTACGTAC", 1, 10, 1, 10});
    pairs.push_back({{op('X', 1)}, "A", "C", 1, 1, 1, 1});                                                 // no M: empty when trimmed
    pairs.push_back({{}, "", "", 0, 0, 0, 0});
    pairs.push_back({{op('I', 2), op('M', 3), op('X', 1), op('M', 2), op('H', 1)}, "ACGTACG", "ttACGaAC", 1, 6, 3, 8});
    pairs.push_back({{op('H', 1), op('I', 2), op('M', 4), op('X', 1), op('D', 1), op('I', 2)}, "qACGTxy", "ttACGTzuv", 2, 5, 3, 6});
    pairs.push_back({{op('M', 3), op('~', 7), op('X', 0), op('M', 0), op('D', 2), op('I', 0), op('M', 4)}, std::string("-| \0abcde", 9),
                     "|- ZZZZ", 1, 9, 1, 7});                                                              // a 0 byte, bars and gaps as bases
    pairs.push_back({{op('D', 3), op('I', 2), op('X', 1), op('H', 12)}, std::string(16, 'q'), "tcg", 0, 0, 0, 0});
    pairs.push_back({{op('I', 5), op('M', 2), op('D', 300), op('M', 1), op('I', 4)}, std::string(303, 'a'), std::string(12, 'c'),
                     1, 303, 6, 8});
    // a window that is NOT where the trimmed-away ops end: only the record says where it is
    pairs.push_back({{op('H', 5), op('M', 2), op('X', 1), op('M', 3), op('H', 2)}, "0123456789abcdef", "uvwxyz", 9, 14, 1, 6});
    which = 1000;
    for (const Pair &p : pairs)
        for (int trim = 0; trim < 2; trim++) {
            which++;
            const uint32_t  len = (uint32_t)p.ops.size();
            uint64_t *const ops = heap_copy(p.ops.data(), len);
            if (!ops) return 2;
            uint32_t first = 0, count = 0;
            cig_range(ops, len, trim != 0, &first, &count);
            std::string want[3];
            naive(p, trim != 0, want);
            if (count == 0u) {
                CHECK(want[0].empty());
                std::free(ops);
                continue;
            }
            // the sequences as one blob of exactly their bytes, query first
            const std::string blob = p.q + p.t;
            AltWindow         w;
            CHECK(alt_window(trim != 0, blob.size(), 0, (uint32_t)p.q.size(), p.q.size(), (uint32_t)p.t.size(), p.qbegin, p.qend, p.tbegin,
                             p.tend, &w));
            const AltSums s = alt_sums(ops + first, count);
            CHECK(alt_fits(s, w));
            CHECK(s.cols == want[0].size() && want[0].size() == want[1].size() && want[1].size() == want[2].size());
            // exactly the bytes the ops consume, exactly the rows
            uint8_t *const q = heap_copy(reinterpret_cast<const uint8_t *>(blob.data()) + w.q_at, (size_t)s.q);
            uint8_t *const t = heap_copy(reinterpret_cast<const uint8_t *>(blob.data()) + w.t_at, (size_t)s.t);
            uint8_t       *rows[3];
            for (uint8_t *&r : rows) r = static_cast<uint8_t *>(std::malloc(s.cols ? (size_t)s.cols : 1));
            if (!q || !t || !rows[0] || !rows[1] || !rows[2]) return 2;
            CHECK(alt_rows_write(ops + first, count, q, t, rows[0], rows[1], rows[2]) == s.cols);
            for (int k = 0; k < 3; k++) CHECK(std::memcmp(rows[k], want[k].data(), (size_t)s.cols) == 0);
            for (uint8_t *r : rows) std::free(r);
            std::free(q), std::free(t), std::free(ops);
        }
    std::printf("altext host test ok\n");
    return 0;
}
