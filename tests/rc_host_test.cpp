// Stand-alone check of wfa_amd/csrc/wfa_rc.hpp (host only): rc_word() -- the one word function behind the kernels' reverse-complement
// staging, the host's gather and wfahip_revcomp_packed -- on heap buffers of EXACTLY (len + 15) / 16 words, so that a read of the
// word below the sequence or of its pad word is an AddressSanitizer finding; every length 1 .. 100, the bits beyond the last base
// all zero and all one, against a base-by-base restatement.  Built under the host sanitizers by tests/test_revcomp_abi.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../wfa_amd/csrc/wfa_rc.hpp"

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            std::fprintf(stderr, "%s:%d: %s  (len %u, word %u)\n", __FILE__, __LINE__, #cond, len, j); \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

int main() {
    using namespace wfa;
    uint32_t len = 0, j = 0;
    // the sixteen groups of a word, reversed
    CHECK(rc_rev2(0x0000001Bu) == 0xE4000000u);  // GTCA and twelve A -> twelve A and ACTG
    CHECK(rc_rev2(0x80000001u) == 0x40000002u);
    uint64_t lcg = 12345;
    for (len = 1; len <= 100; len++) {
        const uint32_t nw = (len + 15u) / 16u;
        for (int fill = 0; fill < 2; fill++) {
            // codes of the sequence, then exactly nw source words on the heap, the tail of the last one zero or all ones
            uint8_t *const  code = static_cast<uint8_t *>(std::malloc(len));
            uint32_t *const src  = static_cast<uint32_t *>(std::malloc(nw * sizeof(uint32_t)));
            uint32_t *const dst  = static_cast<uint32_t *>(std::malloc(nw * sizeof(uint32_t)));
            if (!code || !src || !dst) return 2;
            for (uint32_t w = 0; w < nw; w++) src[w] = fill ? 0xFFFFFFFFu : 0u;
            for (uint32_t i = 0; i < len; i++) {
                lcg     = lcg * 6364136223846793005ull + 1442695040888963407ull;
                code[i] = (uint8_t)((lcg >> 33) & 3u);
                src[i / 16] = (src[i / 16] & ~(3u << (2 * (i % 16)))) | ((uint32_t)code[i] << (2 * (i % 16)));
            }
            for (j = 0; j < nw; j++) dst[j] = rc_word(src, len, j);
            for (j = 0; j < nw; j++) {
                uint32_t want = 0;  // base i of the result: base len - 1 - i of the source, complemented; nothing beyond the last base
                for (uint32_t b = 0; b < 16 && 16 * j + b < len; b++) want |= (uint32_t)(code[len - 1 - (16 * j + b)] ^ 2u) << (2 * b);
                CHECK(dst[j] == want);
            }
            // an involution: the reverse complement of the result (its tail zero) is the source, tail cleared
            for (j = 0; j < nw; j++) {
                uint32_t keep = src[j];
                if (j == nw - 1 && len % 16) keep &= (1u << (2 * (len % 16))) - 1u;
                CHECK(rc_word(dst, len, j) == keep);
            }
            std::free(code), std::free(src), std::free(dst);
        }
    }
    std::printf("rc host test ok\n");
    return 0;
}
