// Stand-alone host program over wfa_amd/csrc/wfa_packdev.hpp, the 16-bytes-to-a-word rule of wfahip_pack_pairs_device, compiled with the
// host compiler alone (tests/test_packdev_host.py; also under -fsanitize=address,undefined).
//   packdev_host_test                 the rule against a byte loop written here: every piece length, every byte value, junk behind
//   packdev_host_test IN OUT          packs the sequences of file IN into file OUT, for the comparison with wfahip_pack_pairs:
//       IN:  per sequence  u32 len, u32 held (>= len, a multiple of 16: the bytes that follow, junk behind the sequence included), bytes
//       OUT: per sequence  u32 bad (0 / 1), then (len + 15) / 16 + 1 words, the last one the zero pad word
#include "../wfa_amd/csrc/wfa_packdev.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace wfa;

static int fails = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);   \
            fails++;                                                  \
        }                                                             \
    } while (0)

static bool is_acgt(uint8_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }

// one piece of 16 held bytes, the first n of which count
static uint32_t piece(const uint8_t *s, uint32_t n, uint32_t *bad) {
    uint32_t d[4];
    std::memcpy(d, s, 16);
    return pkd_word16(d, n, bad);
}

static void selftest() {
    uint32_t seed = 12345u;
    const auto rnd = [&] { return seed = seed * 1664525u + 1013904223u, seed >> 8; };
    // every piece length, ACGT inside, every kind of byte behind
    for (uint32_t n = 1; n <= 16; n++)
        for (int rep = 0; rep < 64; rep++) {
            uint8_t s[16];
            uint32_t want = 0;
            for (uint32_t k = 0; k < 16; k++) {
                s[k] = k < n ? (uint8_t)"ACGT"[rnd() & 3] : (uint8_t)(rep == 0 ? 0xFF : rep == 1 ? 'n' : rep == 2 ? 0 : rnd());
                if (k < n) want |= (uint32_t)((s[k] >> 1) & 3) << (2 * k);
            }
            uint32_t bad = 0;
            CHECK(piece(s, n, &bad) == want);
            CHECK(bad == 0);
        }
    // every byte value at every position of every piece length: the verdict, and the code of the byte
    for (uint32_t n = 1; n <= 16; n++)
        for (uint32_t pos = 0; pos < 16; pos++)
            for (uint32_t v = 0; v < 256; v++) {
                uint8_t s[16];
                std::memset(s, 'G', 16);
                s[pos] = (uint8_t)v;
                uint32_t bad = 0;
                const uint32_t w = piece(s, n, &bad);
                CHECK((bad != 0) == (pos < n && !is_acgt((uint8_t)v)));
                CHECK(((w >> (2 * pos)) & 3u) == (pos < n ? ((v >> 1) & 3u) : 0u));
            }
    // a verdict that is set stays set; n = 0 counts nothing
    uint8_t s[16];
    std::memset(s, 'x', 16);
    uint32_t bad = 0;
    CHECK(pkd_pack4(0x78787878u, 0, &bad) == 0 && bad == 0);
    piece(s, 3, &bad);
    CHECK(bad != 0);
    std::memset(s, 'A', 16);
    piece(s, 16, &bad);
    CHECK(bad != 0);
}

int main(int argc, char **argv) {
    if (argc == 1) {
        selftest();
        if (fails) return 1;
        std::printf("packdev host test ok\n");
        return 0;
    }
    if (argc != 3) return 2;
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t hdr[2];
    while (std::fread(hdr, 4, 2, in) == 2) {
        const uint32_t len = hdr[0], held = hdr[1];
        if (held < len || held % 16 != 0) return 3;
        std::vector<uint8_t> s(held);
        if (held && std::fread(s.data(), 1, held, in) != held) return 3;
        const uint32_t nw = (len + 15) / 16;
        std::vector<uint32_t> w(nw + 2, 0u);  // bad, the words, the pad word
        uint32_t bad = 0;
        for (uint32_t j = 0; j < nw; j++) w[1 + j] = piece(s.data() + 16 * j, len - 16 * j < 16 ? len - 16 * j : 16, &bad);
        w[0] = bad != 0;
        std::fwrite(w.data(), 4, w.size(), out);
    }
    std::fclose(in), std::fclose(out);
    return 0;
}
