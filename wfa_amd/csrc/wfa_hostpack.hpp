// wfa_hostpack.hpp -- the host side's 2-bit packer and the one loop that splits a range of items over host threads.  Plain
// C++17 without a HIP include or type: tests/hostpack_test.cpp compiles it alone, under the host sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

namespace wfa {

// 16 bases -> one word, eight bytes at a time: the codes are (byte >> 1) & 3, gathered by three shift-or steps; a byte
// outside ACGT shows as a difference between the byte and the canonical letter of its code (0x41 + 2 code, + 15 for T).
inline uint32_t pack8(uint64_t w, uint64_t &bad) {
    const uint64_t x = (w >> 1) & 0x0303030303030303ull;
    const uint64_t t = (x >> 1) & ~x & 0x0101010101010101ull;  // code 2 = 'T'
    bad |= (0x4141414141414141ull + 2 * x + 15 * t) ^ w;
    uint64_t y = (x | (x >> 6)) & 0x000F000F000F000Full;
    y          = (y | (y >> 12)) & 0x000000FF000000FFull;
    return (uint32_t)((y | (y >> 24)) & 0xFFFFull);
}
// one sequence -> dst[0 .. (len + 15) / 16] (the last word is the zero pad word); returns true on a byte outside ACGT
inline bool pack_seq_fast(const uint8_t *s, uint32_t len, uint32_t *dst) {
    uint64_t       bad = 0;
    const uint32_t nw = len / 16;
    for (uint32_t w = 0; w < nw; w++) {
        uint64_t a, b;
        std::memcpy(&a, s + 16 * w, 8), std::memcpy(&b, s + 16 * w + 8, 8);
        dst[w] = pack8(a, bad) | (pack8(b, bad) << 16);
    }
    const uint32_t rem = len - 16 * nw;
    if (rem) {
        uint8_t tail[16];
        std::memset(tail, 'A', 16);
        std::memcpy(tail, s + 16 * nw, rem);
        uint64_t a, b;
        std::memcpy(&a, tail, 8), std::memcpy(&b, tail + 8, 8);
        dst[nw] = pack8(a, bad) | (pack8(b, bad) << 16);
        dst[nw + 1] = 0;
    } else {
        dst[nw] = 0;
    }
    return bad != 0;
}

// range(a, b) over [first, last) in contiguous parts of ceil(count / n_threads) items, each part on a thread of its own.  One
// thread: the calling one, none is spawned.  A part whose thread cannot be created runs on the calling thread; an empty part
// calls nothing; all threads are joined before the return.  `range` is copied into each thread and must not throw.
template <class F>
void parallel_ranges(uint64_t first, uint64_t last, unsigned n_threads, F &&range) {
    n_threads = std::max(1u, n_threads);
    const uint64_t           per = (last - first + n_threads - 1) / n_threads;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < n_threads; t++) {
        const uint64_t a = std::min(last, first + (uint64_t)t * per), b = std::min(last, a + per);
        if (b <= a) continue;
        bool inl = n_threads == 1;
        if (!inl) {
            try {
                th.emplace_back(range, a, b);
            } catch (...) {
                inl = true;
            }
        }
        if (inl) range(a, b);
    }
    for (auto &t : th) t.join();
}

// threads of a host-side packing loop: half the hardware threads, at most `cap`, at least one; env: WFAHIP_PACK_THREADS overrides it
inline unsigned host_pack_threads(unsigned cap, bool env) {
    const char *e = env ? std::getenv("WFAHIP_PACK_THREADS") : nullptr;
    if (e) return (unsigned)std::max(1, std::atoi(e));
    return std::max(1u, std::min(cap, std::thread::hardware_concurrency() / 2));
}

}  // namespace wfa
