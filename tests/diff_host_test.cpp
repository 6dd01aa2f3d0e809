// Stand-alone check of wfa_amd/csrc/wfa_diff.hpp (host only): the one rendering rule behind wfa_diff_write_kernel,
// wfa_diff_pk_write_kernel, wfahip_diff_text and wfahip_diff_text_packed.  diff_write, diff_render and diff_op_byte against a naive
// writer that goes column by column over plain strings.  The ops, the bytes, the words and the text each sit in a heap block of
// EXACTLY their size -- a byte or a word touched outside one is an AddressSanitizer finding --, the bits of a sequence's last data
// word beyond its last base and its pad word are random, and the packed query is read on both strands.  Every gap and every X run of
// 1 .. 70 columns starts at every residue 0 .. 15 of a word, with and without bases behind it; then random whole pairs.
// Built plain and under the host sanitizers by tests/test_diff_abi.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../wfa_amd/csrc/wfa_diff.hpp"

#define CHECK(cond)                                                                                              \
    do {                                                                                                         \
        if (!(cond)) {                                                                                           \
            std::fprintf(stderr, "%s:%d: %s  (len %u, at %u, rc %d)\n", __FILE__, __LINE__, #cond, len, at, rc); \
            return 1;                                                                                            \
        }                                                                                                        \
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

static std::string random_bytes(uint32_t n) {
    std::string s(n, 'A');
    for (char &c : s) c = (char)(rnd() & 0xFFu);
    return s;
}

static std::string revcomp(const std::string &s) {
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : 'C';
    return r;
}

static char lower(char c) { return c >= 'A' && c <= 'Z' ? (char)(c + 32) : c; }

// the rule, column by column over the windows' bytes
static std::string naive(const std::vector<uint64_t> &ops, const std::string &q, const std::string &t) {
    std::string out;
    size_t      qp = 0, tp = 0;
    for (uint64_t o : ops) {
        const char     letter = (char)(o >> 32);
        const uint32_t n      = (uint32_t)o;
        if (n == 0) continue;
        if (letter == 'M') {
            out += ':' + std::to_string(n);
            qp += n, tp += n;
        } else if (letter == 'X') {
            for (uint32_t x = 0; x < n; x++) out += '*', out += lower(t[tp++]), out += lower(q[qp++]);
        } else if (letter == 'I') {
            out += '-';
            for (uint32_t x = 0; x < n; x++) out += lower(t[tp++]);
        } else if (letter == 'D' || letter == 'H') {
            out += '+';
            for (uint32_t x = 0; x < n; x++) out += lower(q[qp++]);
        }
    }
    return out;
}

template <class T>
static T *exact(const T *src, size_t n) {  // a heap block of exactly n elements (one byte for none: malloc(0) may be null)
    T *p = static_cast<T *>(std::malloc(n ? n * sizeof(T) : 1));
    if (p && n) std::memcpy(p, src, n * sizeof(T));
    return p;
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

// diff_write and, op by op, diff_render and diff_op_byte over reader S against `want`; 0 if all agree
template <class Seq>
static int same_text(const std::vector<uint64_t> &ops_v, const Seq &S, const std::string &want) {
    using namespace wfa;
    uint64_t *const ops = exact(ops_v.data(), ops_v.size());
    uint8_t *const  dst = static_cast<uint8_t *>(std::malloc(want.size() ? want.size() : 1));
    if (!ops || !dst) return 2;
    int            bad   = 0;
    const uint32_t count = (uint32_t)ops_v.size();
    const DiffSums s     = diff_sums(ops, count);
    if (s.bytes != want.size() || diff_write(ops, count, S, dst) != want.size() || std::memcmp(dst, want.data(), want.size()) != 0) bad = 1;
    uint64_t at = 0, qp = 0, tp = 0;
    for (uint32_t k = 0; k < count && !bad; k++) {
        const uint32_t kind = alt_kind(ops[k]), n = alt_cols(ops[k]);
        const uint64_t nb   = diff_op_bytes(ops[k]);
        if (nb != 0 && !cig_is_m(ops[k]))
            for (uint64_t x = 0; x < nb; x++)
                if (diff_op_byte(kind, S, qp, tp, x) != (uint8_t)want[at + x]) bad = 1;
        at += nb;
        if (kind & ALT_Q) qp += n;
        if (kind & ALT_T) tp += n;
    }
    if (at != want.size() || qp != s.a.q || tp != s.a.t) bad = 1;
    std::free(ops), std::free(dst);
    return bad;
}

// the ops over the windows q_win / t_win, which start at q_at / t_at of sequences with `slack` bases behind the windows: from bytes
// (any byte values) when !acgt, else from bytes and from words on both strands
static int pair_ok(const std::vector<uint64_t> &ops, const std::string &q_win, const std::string &t_win, uint32_t q_at, uint32_t t_at,
                   uint32_t slack, bool acgt) {
    using namespace wfa;
    const std::string want = naive(ops, q_win, t_win);
    {
        uint8_t *const q = exact(reinterpret_cast<const uint8_t *>(q_win.data()), q_win.size());
        uint8_t *const t = exact(reinterpret_cast<const uint8_t *>(t_win.data()), t_win.size());
        if (!q || !t) return 2;
        const int bad = same_text(ops, DiffByteSeq{q, t}, want);
        std::free(q), std::free(t);
        if (bad) return bad;
    }
    if (!acgt) return 0;
    const std::string q_seq = random_acgt(q_at) + q_win + random_acgt(slack), t_seq = random_acgt(t_at) + t_win + random_acgt(slack);
    for (int rc = 0; rc < 2; rc++) {
        uint32_t *const qw = pack_exact(rc ? revcomp(q_seq) : q_seq), *const tw = pack_exact(t_seq);
        if (!qw || !tw) return 2;
        const int bad = same_text(ops, DiffPkSeq{qw, tw, (uint32_t)q_seq.size(), (uint32_t)t_seq.size(), q_at, t_at, rc != 0}, want);
        std::free(qw), std::free(tw);
        if (bad) return bad;
    }
    return 0;
}

int main() {
    using namespace wfa;
    uint32_t len = 0, at = 0;
    int      rc = 0;
    // lower case: every byte value in every byte of a word
    for (uint32_t b = 0; b < 256; b++) {
        len = b;
        CHECK(diff_lc(b) == (uint32_t)(uint8_t)lower((char)b));
        for (at = 0; at < 4; at++) {
            const uint32_t others = rnd(), v = (others & ~(0xFFu << (8 * at))) | (b << (8 * at)), got = diff_lc4(v);
            for (uint32_t j = 0; j < 4; j++) CHECK(((got >> (8 * j)) & 0xFFu) == (uint32_t)(uint8_t)lower((char)(v >> (8 * j))));
        }
    }
    len = 0, at = 0;
    // the bytes of an op, 64 bits wide; an M op reads no base: its reader holds null pointers
    CHECK(diff_op_bytes(op('M', 0)) == 0 && diff_op_bytes(op('X', 0)) == 0 && diff_op_bytes(op('I', 0)) == 0 && diff_op_bytes(op('~', 9)) == 0);
    CHECK(diff_op_bytes(op('M', 7)) == 2 && diff_op_bytes(op('M', 42)) == 3 && diff_op_bytes(op('M', 123)) == 4 && diff_op_bytes(op('M', 4294967295u)) == 11);
    CHECK(diff_op_bytes(op('X', 4294967295u)) == 12884901885ull && diff_op_bytes(op('I', 4294967295u)) == 4294967296ull);
    CHECK(diff_op_bytes(op('D', 1)) == 2 && diff_op_bytes(op('H', 16)) == 17 && diff_op_bytes(op('X', 5)) == 15);
    for (uint32_t count : {7u, 42u, 123u, 1000000007u, 4294967295u}) {
        uint8_t *const dst = static_cast<uint8_t *>(std::malloc(11));
        if (!dst) return 2;
        const std::string want = ':' + std::to_string(count);
        len                    = count;
        CHECK(diff_render(op('M', count), DiffByteSeq{nullptr, nullptr}, 0, 0, dst) == want.size() && std::memcmp(dst, want.data(), want.size()) == 0);
        std::free(dst);
    }
    {
        const DiffSums s = diff_sums(std::vector<uint64_t>{op('X', 4294967295u), op('X', 4294967295u), op('H', 3), op('Z', 5), op('M', 10)}.data(), 5);
        CHECK(s.bytes == 2 * 12884901885ull + 4 + 3 && s.a.q == 2 * 4294967295ull + 13 && s.a.t == 2 * 4294967295ull + 10);
    }
    // the known answer of the reference's README
    {
        const std::vector<uint64_t> ops = {op('M', 1), op('X', 2), op('M', 2), op('X', 1), op('M', 4)};
        CHECK(naive(ops, "ACCATACTCG", "AGGATGCTCG") == ":1*gc*gc:2*ga:4");
        CHECK(pair_ok(ops, "ACCATACTCG", "AGGATGCTCG", 0, 0, 0, true) == 0);
    }
    // one gap or X run of every length 1 .. 70 at every start residue of a word, the window ending with its sequence and not
    for (len = 1; len <= 70; len++)
        for (at = 0; at < 16; at++)
            for (uint32_t slack = 0; slack < 2; slack++)
                for (char letter : {'I', 'D', 'H', 'X'}) {
                    const std::vector<uint64_t> ops = {op('M', at % 3), op(letter, len), op('M', 1)};
                    const AltSums               s   = alt_sums(ops.data(), 3);
                    rc                              = letter;
                    CHECK(pair_ok(ops, random_acgt((uint32_t)s.q), random_acgt((uint32_t)s.t), at, (at * 7u + 3u) % 16u, slack * (1u + at % 5u), true) == 0);
                }
    rc = 0;
    // whole pairs: every letter, counts 0 .. 19, now and then a long op; any byte values from bytes, ACGT from words
    for (int pair = 0; pair < 600; pair++) {
        std::vector<uint64_t> ops;
        const uint32_t        n_ops = 1u + rnd() % 12u;
        for (uint32_t k = 0; k < n_ops; k++) ops.push_back(op("MXIDH~"[rnd() % 6u], rnd() % 20u));
        if (pair % 7 == 0) ops.push_back(op("MXIDH"[rnd() % 5u], 60u + rnd() % 200u));
        const AltSums s    = alt_sums(ops.data(), (uint32_t)ops.size());
        const bool    acgt = pair % 2 == 0;
        len = (uint32_t)s.q, at = (uint32_t)pair;
        CHECK(pair_ok(ops, acgt ? random_acgt((uint32_t)s.q) : random_bytes((uint32_t)s.q), acgt ? random_acgt((uint32_t)s.t) : random_bytes((uint32_t)s.t),
                      rnd() % 20u, rnd() % 20u, rnd() % 3u, acgt) == 0);
    }
    std::printf("diff host test ok\n");
    return 0;
}
