// Stand-alone check of the mirror addressing in wfa_amd/csrc/wfa_rc.hpp (host only): the byte address wfahip_align_batch_packed_rc gives
// the reverse complement of a flagged query.  For every length 1 .. 100 at word offsets 0, 1 and 5, in a heap buffer of EXACTLY the
// words needed and a heap blob of EXACTLY rc_mirror_bytes(n_words) bytes -- a store or a read outside either is an AddressSanitizer
// finding -- every forward word is expanded into its mirror block the way wfa_unpack_pairs_kernel does it; then the len bytes at
// rc_mirror_off must be the byte-wise reverse complement, rc_mirror_word must recover the word offset, and every PREFIX length at
// the same offset must read its own reverse complement from the same mirror.  The bits of the last word beyond the last base are all
// zero and all one.  Built under the host sanitizers by tests/test_align_rc_abi.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../wfa_amd/csrc/wfa_rc.hpp"

#define CHECK(cond)                                                                                                    \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            std::fprintf(stderr, "%s:%d: %s  (len %u, word offset %u, prefix %u)\n", __FILE__, __LINE__, #cond, len, woff, pre); \
            return 1;                                                                                                  \
        }                                                                                                              \
    } while (0)

int main() {
    using namespace wfa;
    static const char LETTER[4] = {'A', 'C', 'T', 'G'};  // code = (ascii >> 1) & 3
    static const uint32_t WOFFS[3] = {0u, 1u, 5u};
    uint32_t len = 0, woff = 0, pre = 0;
    uint64_t lcg = 4321;
    // the addresses: TOP + 1 a multiple of 16, a block 16-byte aligned, forward byte a and Mir(a) = TOP - a inside the blob's two halves
    for (uint64_t nwords = 1; nwords <= 40; nwords++) {
        const uint64_t top = rc_mirror_top(nwords), B = 16 * nwords;
        CHECK(top == 2 * B + 47 && rc_mirror_bytes(nwords) == 2 * B + 96);
        for (uint64_t w = 0; w < nwords; w++) {
            CHECK(rc_mirror_block(top, w) % 16 == 0 && rc_mirror_block(top, w) == 2 * B + 32 - 16 * w);
            CHECK(rc_mirror_block(top, w) >= B + 48 && rc_mirror_block(top, w) + 16 <= rc_mirror_bytes(nwords));
        }
    }
    for (len = 1; len <= 100; len++) {
        const uint32_t nw = (len + 15u) / 16u;
        for (int wi = 0; wi < 3; wi++) {
            woff = WOFFS[wi];
            for (int fill = 0; fill < 2; fill++) {
                const uint64_t  n_words = (uint64_t)woff + nw, top = rc_mirror_top(n_words), bytes = rc_mirror_bytes(n_words);
                uint8_t *const  code  = static_cast<uint8_t *>(std::malloc(len));
                uint32_t *const words = static_cast<uint32_t *>(std::malloc(n_words * sizeof(uint32_t)));
                uint8_t *const  blob  = static_cast<uint8_t *>(std::malloc(bytes));
                if (!code || !words || !blob) return 2;
                std::memset(blob, '#', bytes);
                for (uint64_t w = 0; w < n_words; w++) {  // (the words below the sequence: other sequences' bases)
                    lcg      = lcg * 6364136223846793005ull + 1442695040888963407ull;
                    words[w] = w < woff ? (uint32_t)(lcg >> 32) : (fill ? 0xFFFFFFFFu : 0u);
                }
                for (uint32_t i = 0; i < len; i++) {
                    lcg     = lcg * 6364136223846793005ull + 1442695040888963407ull;
                    code[i] = (uint8_t)((lcg >> 33) & 3u);
                    uint32_t &w = words[woff + i / 16];
                    w = (w & ~(3u << (2 * (i % 16)))) | ((uint32_t)code[i] << (2 * (i % 16)));
                }
                // every forward word into its mirror block: one aligned 16-byte store
                for (uint64_t w = 0; w < n_words; w++) {
                    uint32_t o[4];
                    rc_mirror_letters(words[w], o);
                    std::memcpy(blob + rc_mirror_block(top, w), o, 16);
                }
                // the sequence and every prefix of it, at the same word offset, from the same mirror
                for (pre = 1; pre <= len; pre++) {
                    const uint64_t off = rc_mirror_off(top, woff, pre);
                    CHECK(off == 2 * 16 * n_words + 48 - 16ull * woff - pre);
                    CHECK(off >= 16 * n_words + 48 && off + pre <= top + 1);
                    CHECK(rc_mirror_word(top, off, pre) == woff);
                    for (uint32_t i = 0; i < pre; i++) CHECK(blob[off + i] == (uint8_t)LETTER[code[pre - 1 - i] ^ 2u]);
                }
                // nothing was stored outside the mirror blocks of the words
                for (uint64_t a = 0; a < rc_mirror_block(top, n_words - 1); a++) CHECK(blob[a] == '#');
                for (uint64_t a = top + 1; a < bytes; a++) CHECK(blob[a] == '#');
                std::free(code), std::free(words), std::free(blob);
            }
        }
    }
    std::printf("rc mirror host test ok\n");
    return 0;
}
