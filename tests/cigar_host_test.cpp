// Stand-alone check of wfa_amd/csrc/wfa_cigar.hpp (host only): the one rendering rule behind the CIGAR text kernels and
// wfahip_cigar_text.  Every count at which the number of digits changes, and the trim cases of trimOps, are rendered into heap
// buffers of EXACTLY the computed size, so that a byte written past the text -- or an op read outside the pair's ops, which lie in
// a buffer of exactly their number -- is an AddressSanitizer finding; the text is compared with snprintf's.  Built under the host
// sanitizers by tests/test_cigar_abi.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../wfa_amd/csrc/wfa_cigar.hpp"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "%s:%d: %s  (case %d)\n", __FILE__, __LINE__, #cond, which); \
            return 1;                                                            \
        }                                                                        \
    } while (0)

static uint64_t op(char letter, uint32_t count) { return ((uint64_t)(uint8_t)letter << 32) | count; }

// the restatement: printf's decimal and the letter, over the ops from the first M to the last M when trimmed
static std::string naive(const std::vector<uint64_t> &ops, bool trim) {
    size_t a = 0, b = ops.size();
    if (trim) {
        while (a < b && (ops[a] >> 32) != 'M') a++;
        while (b > a && (ops[b - 1] >> 32) != 'M') b--;
    }
    std::string s;
    for (size_t k = a; k < b; k++) {
        char buf[16];
        std::snprintf(buf, sizeof buf, "%u%c", (unsigned)(ops[k] & 0xFFFFFFFFu), (char)(ops[k] >> 32));
        s += buf;
    }
    return s;
}

int main() {
    using namespace wfa;
    int which = 0;
    const uint32_t counts[] = {0u, 1u, 9u, 10u, 99u, 100u, 999u, 1000u, 9999u, 10000u, 99999u, 100000u, 999999u, 1000000u, 9999999u,
                               10000000u, 99999999u, 100000000u, 999999999u, 1000000000u, 4294967295u};
    const char letters[] = {'M', 'D', 'I', 'X', 'H', '~'};
    // one op at a time: its length, and its text in a buffer of exactly that length
    for (uint32_t c : counts)
        for (char l : letters) {
            which++;
            char want[16];
            const int wl = std::snprintf(want, sizeof want, "%u%c", (unsigned)c, l);
            CHECK(cig_digits(c) == (uint32_t)wl - 1u);
            CHECK(cig_op_bytes(op(l, c)) == (uint32_t)wl);
            uint8_t *const dst = static_cast<uint8_t *>(std::malloc((size_t)wl));
            if (!dst) return 2;
            CHECK(cig_render(op(l, c), dst) == (uint32_t)wl);
            CHECK(std::memcmp(dst, want, (size_t)wl) == 0);
            std::free(dst);
        }
    CHECK(CIG_MAX_OP_BYTES == cig_op_bytes(op('M', 4294967295u)));
    // whole pairs, both trim modes
    std::vector<std::vector<uint64_t>> cases;
    {
        std::vector<uint64_t> all;
        for (size_t i = 0; i < sizeof counts / sizeof counts[0]; i++) all.push_back(op(letters[i % 6], counts[i]));
        cases.push_back(all);
    }
    cases.push_back({});                                                                         // no op
    cases.push_back({op('X', 1)});                                                               // no M: empty when trimmed
    cases.push_back({op('D', 3), op('I', 2), op('X', 1), op('H', 12)});                          // no M, several ops
    cases.push_back({op('M', 150)});                                                             // a single op M
    cases.push_back({op('M', 5), op('X', 1), op('I', 2), op('D', 3), op('H', 4)});               // M only first
    cases.push_back({op('I', 1), op('D', 2), op('X', 3), op('H', 1), op('M', 7)});               // M only last
    cases.push_back({op('I', 10), op('D', 2), op('X', 3), op('H', 100), op('M', 7), op('X', 1), op('M', 99), op('H', 1), op('X', 1),
                     op('D', 1000), op('I', 9)});                                                // leading and trailing runs
    cases.push_back({op('M', 1), op('D', 1), op('I', 22), op('X', 333), op('H', 4444), op('~', 5), op('M', 2)});  // all between two M kept
    which = 1000;
    for (const auto &ops : cases)
        for (int trim = 0; trim < 2; trim++) {
            which++;
            const uint32_t  len  = (uint32_t)ops.size();
            uint64_t *const heap = static_cast<uint64_t *>(std::malloc(len ? len * sizeof(uint64_t) : 1));  // exactly the pair's ops
            if (!heap) return 2;
            if (len) std::memcpy(heap, ops.data(), len * sizeof(uint64_t));
            uint32_t first = 0, count = 0;
            cig_range(heap, len, trim != 0, &first, &count);
            CHECK(first <= len && count <= len - first);
            const std::string want  = naive(ops, trim != 0);
            const uint64_t    bytes = cig_text_bytes(heap + first, count);
            CHECK(bytes == want.size());
            uint8_t *const dst = static_cast<uint8_t *>(std::malloc(bytes ? (size_t)bytes : 1));  // exactly the text
            if (!dst) return 2;
            CHECK(cig_text_write(heap + first, count, dst) == bytes);
            CHECK(std::memcmp(dst, want.data(), (size_t)bytes) == 0);
            if (trim && count) CHECK(cig_is_m(heap[first]) && cig_is_m(heap[first + count - 1]));
            std::free(dst), std::free(heap);
        }
    std::printf("cigar host test ok\n");
    return 0;
}
