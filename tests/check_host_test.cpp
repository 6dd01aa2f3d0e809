// Stand-alone check of wfa_amd/csrc/wfa_check.hpp (host only): the one rule behind the check kernels and wfahip_check_alignments.
// Every pair is judged from heap copies of EXACTLY its ops, EXACTLY its sequences' bytes and EXACTLY its sequences' words (data
// words and the pad word), so that an op, a base or a word read outside them is an AddressSanitizer finding; the eight words are
// compared with a column-by-column restatement, over bytes and over words of both strands.  Built plain and under the host
// sanitizers by tests/test_check_abi.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../wfa_amd/csrc/wfa_check.hpp"

using namespace wfa;

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
    std::string           q, t;  // ACGT
    ChkRec                rec;
    bool                  seq_ok;
};

static bool in(uint32_t l, const char *set) { return l < 128u && l != 0u && std::strchr(set, (int)l) != nullptr; }

// the restatement: one column at a time, sums as unsigned __int128
static void naive(const Pair &p, const ChkRule &R, bool packed, uint32_t out[8]) {
    typedef unsigned __int128 u128;
    const size_t n = p.ops.size();
    uint32_t     f = 0;
    u128         cost = 0, qu = 0, tu = 0, col = 0, n_bad = 0, first = ~(u128)0;
    size_t       m0 = n, m1 = 0;
    for (size_t k = 0; k < n; k++) {
        const uint32_t l = (uint32_t)(p.ops[k] >> 32), c = (uint32_t)p.ops[k];
        if (!in(l, "MXIDH")) f |= CHK_LETTER;
        if (c == 0) f |= CHK_ZERO;
        if (k && l == (uint32_t)(p.ops[k - 1] >> 32)) f |= CHK_UNMERGED;
        if (l == 'M') m0 = m0 == n ? k : m0, m1 = k + 1;
        if (l == 'X') cost += (u128)R.x * c;
        if (in(l, "IDH")) cost += (u128)R.o + (u128)R.e * c;
        if (p.seq_ok && in(l, "MX"))
            for (uint32_t x = 0; x < c && qu + x < p.q.size() && tu + x < p.t.size(); x++) {
                const bool differ = p.q[(size_t)(qu + x)] != p.t[(size_t)(tu + x)];
                if (differ == (l == 'M')) {
                    f |= l == 'M' ? CHK_M_DIFFERS : CHK_X_EQUAL;
                    if (n_bad++ == 0) first = col + x;
                }
            }
        if (in(l, "MXIDH")) col += c;
        if (in(l, "MXDH")) qu += c;
        if (in(l, "MXI")) tu += c;
    }
    if (m1 == 0) f |= CHK_NO_M, m0 = 0;
    if (!p.seq_ok) f |= CHK_SEQ_RANGE;
    if (qu > p.q.size()) f |= CHK_Q_OVER;
    if (qu < p.q.size()) f |= CHK_Q_UNDER;
    if (tu > p.t.size()) f |= CHK_T_OVER;
    if (tu < p.t.size()) f |= CHK_T_UNDER;
    for (int trim = 0; trim < 2; trim++) {
        const size_t a = trim ? m0 : 0, b = trim ? m1 : n;
        u128         qs = 0, ts = 0, cs = 0;
        for (size_t k = a; k < b; k++) {
            const uint32_t l = (uint32_t)(p.ops[k] >> 32), c = (uint32_t)p.ops[k];
            if (in(l, "MXIDH")) cs += c;
            if (in(l, "MXDH")) qs += c;
            if (in(l, "MXI")) ts += c;
        }
        if (b <= a || (packed && cs == 0)) continue;
        bool   ok = p.seq_ok;
        int64_t qn = (int64_t)p.q.size(), tn = (int64_t)p.t.size();
        if (ok && trim) {
            ok = p.rec.qbegin >= 1 && p.rec.qbegin - 1 <= p.rec.qend && p.rec.qend <= qn && p.rec.tbegin >= 1 && p.rec.tbegin - 1 <= p.rec.tend &&
                 p.rec.tend <= tn;
            qn = (int64_t)p.rec.qend - p.rec.qbegin + 1, tn = (int64_t)p.rec.tend - p.rec.tbegin + 1;
        }
        if (!ok || qs > (u128)qn || ts > (u128)tn) f |= trim ? CHK_NO_ROWS_TRIMMED : CHK_NO_ROWS;
    }
    if (R.global) {
        if (cost > p.rec.score) f |= CHK_COST_OVER;
        if (cost < p.rec.score) f |= CHK_COST_UNDER;
    }
    uint32_t alen = 0, matches = 0, gaps = 0, regions = 0;
    for (size_t k = m0; k < (m1 ? m1 : (n ? 1 : 0)); k++) {
        const uint32_t l = (uint32_t)(p.ops[k] >> 32), c = (uint32_t)p.ops[k];
        alen += c;
        if (l == 'M') matches += c;
        if (l == 'I' || l == 'D') gaps += c, regions++;
    }
    if (alen != p.rec.align_len) f |= CHK_STAT_ALIGN_LEN;
    if (matches != p.rec.matches) f |= CHK_STAT_MATCHES;
    if (gaps != p.rec.gaps) f |= CHK_STAT_GAPS;
    if (regions != p.rec.gap_regions) f |= CHK_STAT_GAP_REGIONS;
    const u128 cap = 0xFFFFFFFFu;
    out[0] = f, out[1] = (uint32_t)(cost < cap ? cost : cap), out[2] = (uint32_t)(qu < cap ? qu : cap), out[3] = (uint32_t)(tu < cap ? tu : cap);
    out[4] = (uint32_t)(n_bad < cap ? n_bad : cap);
    out[5] = first == ~(u128)0 ? 0xFFFFFFFFu : (uint32_t)(first < cap - 1 ? first : cap - 1);
    out[6] = out[7] = 0;
}

static std::vector<uint32_t> pack(const std::string &s, uint32_t junk) {  // data words and the pad word, junk in the tail bits and the pad
    std::vector<uint32_t> w((s.size() + 15) / 16 + 1, junk);
    for (size_t k = 0; k < s.size(); k++) {
        const uint32_t code = ((uint8_t)s[k] >> 1) & 3u;
        w[k / 16] = (w[k / 16] & ~(3u << (2 * (k % 16)))) | (code << (2 * (k % 16)));
    }
    return w;
}

static std::string revcomp(const std::string &s) {
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : 'C';
    return r;
}

static uint32_t rnd_state = 12345u;
static uint32_t rnd() { return rnd_state = rnd_state * 1664525u + 1013904223u, rnd_state >> 8; }

int main() {
    int                which = 0;
    const ChkRule      rules[3] = {{4, 6, 2, true}, {4, 6, 2, false}, {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, true}};
    std::vector<Pair>  pairs;
    const char         letters[] = "MXIDH~";
    // random op lists over random sequences: most flags come up by themselves; counts of 0 and of 0xFFFFFFFF among them
    for (int k = 0; k < 400; k++) {
        Pair         p;
        const size_t n = k < 4 ? (size_t)k : rnd() % 12;
        for (size_t j = 0; j < n; j++) {
            const uint32_t r = rnd() % 40;
            p.ops.push_back(op(letters[rnd() % (k % 5 ? 5 : 6)], r == 0 ? 0u : r == 1 ? 0xFFFFFFFFu : rnd() % 9));
        }
        const size_t ql = rnd() % 48, tl = rnd() % 48;
        for (size_t j = 0; j < ql; j++) p.q.push_back("ACGT"[rnd() % (k % 3 ? 4 : 2)]);
        for (size_t j = 0; j < tl; j++) p.t.push_back("ACGT"[rnd() % (k % 3 ? 4 : 2)]);
        p.rec    = ChkRec{rnd() % 64, rnd() % 32, rnd() % 32, rnd() % 8, rnd() % 4, (int32_t)(rnd() % 4), (int32_t)(rnd() % 50), (int32_t)(rnd() % 4) - 1,
                       (int32_t)(rnd() % 50)};
        p.seq_ok = k % 7 != 0;
        pairs.push_back(p);
    }
    // consistent pairs: the sequences made from the ops, the record from the restatement's own sums -> no flag at all
    for (int k = 0; k < 40; k++) {
        Pair   p;
        char   prev = 0;
        size_t n = 1 + rnd() % 10;
        for (size_t j = 0; j < n; j++) {
            char l = (j == 0 || j + 1 == n) ? 'M' : letters[rnd() % 5];
            if (l == prev) l = l == 'M' ? 'X' : 'M';
            const uint32_t c = 1 + rnd() % 20;
            p.ops.push_back(op(l, c));
            prev = l;
            for (uint32_t x = 0; x < c; x++) {
                const char b = "ACGT"[rnd() % 4], o = "ACGT"[(std::strchr("ACGT", b) - "ACGT" + 1 + rnd() % 3) % 4];
                if (l == 'M') p.q.push_back(b), p.t.push_back(b);
                if (l == 'X') p.q.push_back(b), p.t.push_back(o);
                if (l == 'I') p.t.push_back(b);
                if (l == 'D' || l == 'H') p.q.push_back(b);
            }
        }
        p.seq_ok = true;
        p.rec    = ChkRec{0, 0, 0, 0, 0, 1, (int32_t)p.q.size(), 1, (int32_t)p.t.size()};
        uint32_t w[8];
        naive(p, rules[0], false, w);  // its cost and, through the flags, nothing else; the stats come from a second look
        p.rec.score = w[1];
        for (uint32_t a = 0; a < 400 && (w[0] & (CHK_STAT_ALIGN_LEN | CHK_STAT_MATCHES | CHK_STAT_GAPS | CHK_STAT_GAP_REGIONS)); a++) {
            if (w[0] & CHK_STAT_ALIGN_LEN) p.rec.align_len++;
            if (w[0] & CHK_STAT_MATCHES) p.rec.matches++;
            if (w[0] & CHK_STAT_GAPS) p.rec.gaps++;
            if (w[0] & CHK_STAT_GAP_REGIONS) p.rec.gap_regions++;
            naive(p, rules[0], false, w);
        }
        if (w[0] != 0u) {
            std::fprintf(stderr, "a consistent pair raises %#x by the restatement (case %d)\n", w[0], k);
            return 1;
        }
        pairs.push_back(p);
    }
    uint32_t seen = 0;
    for (const Pair &p : pairs) {
        uint64_t *ops = heap_copy(p.ops.data(), p.ops.size());
        uint8_t  *q   = heap_copy(reinterpret_cast<const uint8_t *>(p.q.data()), p.q.size());
        uint8_t  *t   = heap_copy(reinterpret_cast<const uint8_t *>(p.t.data()), p.t.size());
        const uint32_t ql = (uint32_t)p.q.size(), tl = (uint32_t)p.t.size(), len = (uint32_t)p.ops.size();
        for (const ChkRule &R : rules) {
            uint32_t want[8], got[8];
            // bytes: a blob of exactly the two sequences' sizes stands for each of them (off 0); a bad range is a blob too short
            naive(p, R, false, want);
            const auto win_q = [&](bool trim, AltWindow *w) {
                return alt_window_1(trim, p.seq_ok ? ql : (uint64_t)ql - 1u + (ql == 0u), 0, ql + (ql == 0u && !p.seq_ok), p.rec.qbegin, p.rec.qend, &w->q_at,
                                    &w->q_n) &&
                       alt_window_1(trim, tl, 0, tl, p.rec.tbegin, p.rec.tend, &w->t_at, &w->t_n);
            };
            if (ql != 0u || p.seq_ok) {  // (an empty query cannot leave a blob by its length)
                chk_pair<false>(R, p.rec, ops, len, ql, tl, win_q, [&]() { return ChkByteSeq{q, t}; }, got);
                CHECK(std::memcmp(got, want, sizeof got) == 0);
                seen |= got[0];
            }
            // words, forward and flagged
            for (int rc = 0; rc < 2; rc++) {
                const std::vector<uint32_t> qw0 = pack(rc ? revcomp(p.q) : p.q, rnd() | (rnd() << 24)), tw0 = pack(p.t, rnd() | (rnd() << 24));
                uint32_t *qw = heap_copy(qw0.data(), qw0.size()), *tw = heap_copy(tw0.data(), tw0.size());
                naive(p, R, true, want);
                const auto win_pk = [&](bool trim, AltWindow *w) {
                    return alt_pk_window_1(trim, qw0.size() - (p.seq_ok ? 0u : 1u), 0, ql, p.rec.qbegin, p.rec.qend, &w->q_at, &w->q_n) &&
                           alt_pk_window_1(trim, tw0.size(), 0, tl, p.rec.tbegin, p.rec.tend, &w->t_at, &w->t_n);
                };
                chk_pair<true>(R, p.rec, ops, len, ql, tl, win_pk, [&]() { return ChkPkSeq{qw, tw, ql, tl, rc != 0}; }, got);
                CHECK(std::memcmp(got, want, sizeof got) == 0);
                std::free(qw), std::free(tw);
            }
        }
        std::free(ops), std::free(q), std::free(t);
        which++;
    }
    // every flag but OPS_RANGE (the entries' own step) came up
    if ((seen | CHK_OPS_RANGE) != CHK_ALL) {
        std::fprintf(stderr, "flags never raised: %#x\n", CHK_ALL & ~(seen | CHK_OPS_RANGE));
        return 1;
    }
    // the pieces at their edges
    {
        uint32_t w[8];
        chk_unread(true, w);
        CHECK(w[0] == (CHK_OPS_RANGE | CHK_NO_ROWS | CHK_NO_ROWS_TRIMMED) && w[1] == 0 && w[7] == 0);
        chk_unread(false, w);
        CHECK(w[0] == 0);
        CHECK(chk_ops_range(0, 1, 0) && chk_ops_range(5, 0, 4) && !chk_ops_range(4, 0, 4) && !chk_ops_range(0, 0, 0) && chk_ops_range(~0ull, 2, 9));
        CHECK(chk_sat_add(~0ull - 1, 1) == ~0ull && chk_sat_add(~0ull, 5) == ~0ull && chk_sat_add(3, 4) == 7);
        CHECK(chk_op_cost(op('D', 0xFFFFFFFFu), rules[2]) == 0xFFFFFFFF00000000ull && chk_op_cost(op('M', 9), rules[2]) == 0);
        CHECK(chk_valid(10, 5, 0, 8, 100) == 3 && chk_valid(10, 8, 0, 8, 100) == 0 && chk_valid(10, 1ull << 40, 0, 8, 100) == 0 &&
              chk_valid(2, 0, 0, 8, 100) == 2);
        CHECK(chk_pass(4, CHK_ALL, CHK_ALL) == 4 && chk_pass(0, CHK_NO_M, CHK_NO_ROWS) == 0 && chk_pass(0, CHK_NO_M, CHK_NO_M) == CHK_PAIR_FAILED);
    }
    std::printf("check host test ok: %d pairs x 3 rules, bytes and words of both strands\n", which);
    return 0;
}
