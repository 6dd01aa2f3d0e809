// Host-only checks of wfa_amd/csrc/wfa_hostpack.hpp: the 2-bit packer against a per-base loop, the thread-splitting loop, the
// thread-count rule.  Built by tests/test_hostpack.py under the address + undefined and the thread sanitizer; exit status 0 = pass.
#include "../wfa_amd/csrc/wfa_hostpack.hpp"

#include <atomic>
#include <cstdio>
#include <memory>

using namespace wfa;

static int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
            failures++;                                    \
        }                                                  \
    } while (0)

// the codes of `len` bases, (byte >> 1) & 3, sixteen per word from bit 0 up; 'A' (code 0) behind the end; then the zero pad word
static std::vector<uint32_t> naive_pack(const uint8_t *s, uint32_t len) {
    std::vector<uint32_t> w(len / 16 + (len % 16 ? 2 : 1), 0u);
    for (uint32_t i = 0; i < len; i++) w[i / 16] |= (uint32_t)((s[i] >> 1) & 3u) << (2 * (i % 16));
    return w;
}

static void check_pack(uint32_t len, int64_t odd_at, uint8_t odd) {
    // (exactly len bytes on the heap: a read past the end is the address sanitizer's to catch)
    std::unique_ptr<uint8_t[]> src(new uint8_t[len]);
    uint32_t                   x = 12345u + len;
    for (uint32_t i = 0; i < len; i++) x = x * 1664525u + 1013904223u, src[i] = (uint8_t)"ACGT"[x >> 30];
    if (odd_at >= 0) src[odd_at] = odd;
    const std::vector<uint32_t> want = naive_pack(src.get(), len);
    std::vector<uint32_t>       got(want.size() + 1, 0xDEADBEEFu);  // (one guard word behind the pad word)
    const bool                  bad = pack_seq_fast(src.get(), len, got.data());
    CHECK(bad == (odd_at >= 0), "len %u odd byte 0x%02x at %lld: returned %d", len, odd, (long long)odd_at, (int)bad);
    // (a byte outside ACGT still packs as its (byte >> 1) & 3: the caller drops the sequence, the words are defined all the same)
    for (size_t w = 0; w < want.size(); w++) CHECK(got[w] == want[w], "len %u word %zu: 0x%08x, want 0x%08x", len, w, got[w], want[w]);
    CHECK(got[want.size() - 1] == 0u, "len %u: the pad word is 0x%08x", len, got[want.size() - 1]);
    CHECK(got[want.size()] == 0xDEADBEEFu, "len %u: a word behind the pad word was written", len);
}

static void test_pack() {
    for (const uint32_t len : {0u, 1u, 15u, 16u, 17u, 31u, 32u, 33u, 2047u}) {
        check_pack(len, -1, 0);
        if (len == 0) continue;
        for (const uint8_t odd : {(uint8_t)'N', (uint8_t)'c', (uint8_t)0x80, (uint8_t)0xC7})
            for (const int64_t at : {(int64_t)0, (int64_t)len / 2, (int64_t)len - 1}) check_pack(len, at, odd);
    }
}

static void test_parallel_ranges() {
    const std::thread::id me = std::this_thread::get_id();
    for (const uint64_t count : {0ull, 1ull, 7ull, 1000ull})
        for (const unsigned nt : {1u, 3u, 16u, 64u})
            for (const uint64_t first : {0ull, 5ull}) {
                std::vector<uint32_t> seen(count, 0u);
                std::atomic<int>      calls{0}, empty{0}, off_thread{0}, unordered{0};
                parallel_ranges(first, first + count, nt, [&](uint64_t a, uint64_t b) {
                    calls++;
                    if (b <= a) empty++;
                    if (a < first || b > first + count) unordered++;
                    if (std::this_thread::get_id() != me) off_thread++;
                    for (uint64_t i = a; i < b; i++) seen[i - first]++;  // (each index belongs to one part: no two threads write a slot)
                });
                uint64_t wrong = 0;
                for (const uint32_t v : seen) wrong += v != 1u;
                CHECK(wrong == 0, "count %llu threads %u: %llu indices not visited exactly once", (unsigned long long)count, nt, (unsigned long long)wrong);
                CHECK(empty == 0 && unordered == 0, "count %llu threads %u: %d empty parts, %d outside the range", (unsigned long long)count, nt, empty.load(), unordered.load());
                CHECK(calls <= (int)nt && (count == 0) == (calls == 0), "count %llu threads %u: %d calls", (unsigned long long)count, nt, calls.load());
                if (nt == 1) CHECK(off_thread == 0, "count %llu: one thread asked for, yet a part ran off the calling thread", (unsigned long long)count);
            }
}

static void test_threads() {
    unsetenv("WFAHIP_PACK_THREADS");
    for (const unsigned cap : {1u, 16u, 64u})
        for (const bool env : {false, true}) {
            const unsigned n = host_pack_threads(cap, env);
            CHECK(n >= 1 && n <= cap, "cap %u: %u threads", cap, n);
        }
    const unsigned plain = host_pack_threads(16, false);
    setenv("WFAHIP_PACK_THREADS", "3", 1);
    CHECK(host_pack_threads(16, true) == 3, "WFAHIP_PACK_THREADS=3 gives %u", host_pack_threads(16, true));
    CHECK(host_pack_threads(2, true) == 3, "the variable is not capped: %u", host_pack_threads(2, true));
    CHECK(host_pack_threads(16, false) == plain, "the variable is read without env: %u, was %u", host_pack_threads(16, false), plain);
    setenv("WFAHIP_PACK_THREADS", "0", 1);
    CHECK(host_pack_threads(16, true) == 1, "WFAHIP_PACK_THREADS=0 gives %u", host_pack_threads(16, true));
    unsetenv("WFAHIP_PACK_THREADS");
}

int main() {
    test_pack();
    test_parallel_ranges();
    test_threads();
    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("hostpack ok\n");
    return failures ? 1 : 0;
}
