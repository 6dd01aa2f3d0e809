// wfa_duo.hpp -- kernel E: blocked register-window forward kernel with a VARIABLE number of lanes per pair.
//
// wfa_blk_kernel<16,1> gives every pair a 64-diagonal window (16 lanes x 4 diagonals), because almost every 1 kbp pair
// needs that many diagonals at SOME score -- but the union of the rows a step reads spans 17 diagonals on average and
// 27 or fewer in 87 % of the pair-steps (oracle band traces, scripts/sim_rows.py): 72 % of the window slots idle.
// Here a 16-lane DPP row holds either ONE pair with a 64-diagonal window or TWO pairs with 32-diagonal windows (8 lanes
// x 4 diagonals each), and a pair changes between the two forms while it runs:
//   * widen   -- a narrow pair whose band outgrows 32 diagonals takes the other half of its row.  If another pair runs
//                there, that pair is PARKED: its rings (6 rows x 32 diagonals) and scalars go to an LDS record of the
//                wave, its packed sequences stay where they are, and it resumes in the next free half of the wave.
//   * narrow  -- a wide pair whose band has shrunk to <= 18 diagonals gives one half of its row back.
//   * recentre-- a pair whose newest row touches the edge of its window is moved so that its band sits in the middle.
// All three are ONE operation: every lane of the wave names the lane its ring registers come from (or none), and 24
// ds_bpermute_b32 move the rings (the LDS crossbar: no LDS memory, no bank conflicts).  It replaces the one-lane DPP
// window shifts of wfa_blk_kernel.
//
// Replaying the band traces through this scheme (scripts/sim_rows.py: four rows, park area of three, the policy
// above) gives 1.73x fewer wave-steps per pair, 1.9 parks per pair and 1.8 % of the pairs handed on because the park
// area is full when they need to widen (they go to the 256-diagonal rung like any pair whose band leaves the window).
//
// With twice the pairs per wave a refill is twice as frequent per wave step, and parked pairs resume ~2 times per
// pair: the refill chain of wfa_blk_kernel (queue atomic -> lengths / offsets -> bytes -> 2-bit packing; three dependent
// round trips during which all pairs of the wave stand still) would eat the gain.  So
//   * the chunk's sequences are 2-bit packed up front by wfa_prepack_kernel (slot = {n, m, status, 0, q words, t words}),
//   * every wave PREFETCHES its next pair one stage per loop iteration -- queue atomic; a step later the slot's words
//     into four registers per lane; a step later those registers into a spare LDS buffer -- so a result is only
//     consumed a whole score step after its request was issued, and a freed half starts its next pair from LDS,
//   * a parked pair resumes from LDS.
//
// Everything else -- the rejection-free WF_NEXT with the decisions shifted in under the offset, the first-window +
// candidate-at-a-time WF_EXTEND, the branch-free band / wf-adaptive reductions, the arena tiles of 8 scores x 64
// diagonals (here with 16-bit words, CompactView fmt 7) and pair_meta for wfa_backtrace_kernel -- is wfa_blk_kernel's,
// with the group size a per-lane value instead of a template argument.  Results do not depend on which pairs share a
// wave: the band of a row is a function of the pair alone as long as its window holds it, and a pair whose band cannot
// be held is handed on (ST_REDO_BAND) and recomputed from scratch by the retry rung.
#pragma once
#include "wfa_blk.hpp"
#include "wfa_duo_cfg.hpp"
#include "wfa_pk16.hpp"

namespace wfa {

// Group reductions: three butterfly stages inside the 8 lanes of a half row, and a fourth (row_mirror) that only the lanes
// of a 16-lane pair execute: EXEC is narrowed to the wave's wide pairs for it (wm = ballot of `wide`; both halves of a wide
// pair are in the mask, so every active lane's mirror partner is active too).  Round 6: before, the fourth stage ran on a
// copy in all lanes and a select kept it for the wide ones -- two more vector instructions per reduced value, ten per step.
// (wait states: a DPP source written by the previous stage is read at least two instructions later; EXEC is written by
// the scalar unit, which a DPP instruction need not wait for.)
struct DuoRed {
#define WFA_DUO_3(opa, opb, opc)                                                                                    \
    unsigned long long sv;                                                                                          \
    asm volatile("s_nop 1\n\t" opa " %0, %0, %0 " WFA_DPP_CTL_XOR1 "\n\t" opb " %1, %1, %1 " WFA_DPP_CTL_XOR1 "\n\t" opc \
        " %2, %2, %2 " WFA_DPP_CTL_XOR1 "\n\t" opa " %0, %0, %0 " WFA_DPP_CTL_XOR2 "\n\t" opb " %1, %1, %1 "        \
        WFA_DPP_CTL_XOR2 "\n\t" opc " %2, %2, %2 " WFA_DPP_CTL_XOR2 "\n\t" opa " %0, %0, %0 " WFA_DPP_CTL_HMIR "\n\t" \
        opb " %1, %1, %1 " WFA_DPP_CTL_HMIR "\n\t" opc " %2, %2, %2 " WFA_DPP_CTL_HMIR "\n\t"                         \
        "s_and_saveexec_b64 %3, %4\n\t" opa " %0, %0, %0 " WFA_DPP_CTL_MIR "\n\t" opb " %1, %1, %1 " WFA_DPP_CTL_MIR    \
        "\n\t" opc " %2, %2, %2 " WFA_DPP_CTL_MIR "\n\ts_mov_b64 exec, %3"                                            \
        : "+v"(a), "+v"(b), "+v"(c), "=&s"(sv)                                                                      \
        : "s"(wm)                                                                                                   \
        : "scc");
#define WFA_DUO_2(opa, opb)                                                                                         \
    unsigned long long sv;                                                                                          \
    asm volatile("s_nop 1\n\t" opa " %0, %0, %0 " WFA_DPP_CTL_XOR1 "\n\t" opb " %1, %1, %1 " WFA_DPP_CTL_XOR1 "\n\ts_nop 0\n\t" \
        opa " %0, %0, %0 " WFA_DPP_CTL_XOR2 "\n\t" opb " %1, %1, %1 " WFA_DPP_CTL_XOR2 "\n\ts_nop 0\n\t" opa        \
        " %0, %0, %0 " WFA_DPP_CTL_HMIR "\n\t" opb " %1, %1, %1 " WFA_DPP_CTL_HMIR "\n\t"                            \
        "s_and_saveexec_b64 %2, %3\n\t" opa " %0, %0, %0 " WFA_DPP_CTL_MIR "\n\t" opb " %1, %1, %1 " WFA_DPP_CTL_MIR    \
        "\n\ts_mov_b64 exec, %2"                                                                                    \
        : "+v"(a), "+v"(b), "=&s"(sv)                                                                               \
        : "s"(wm)                                                                                                   \
        : "scc");
#define WFA_DUO_1(opa)                                                                                              \
    unsigned long long sv;                                                                                          \
    asm volatile("s_nop 1\n\t" opa " %0, %0, %0 " WFA_DPP_CTL_XOR1 "\n\ts_nop 1\n\t" opa " %0, %0, %0 " WFA_DPP_CTL_XOR2 \
        "\n\ts_nop 1\n\t" opa " %0, %0, %0 " WFA_DPP_CTL_HMIR "\n\t"                                                \
        "s_and_saveexec_b64 %1, %2\n\ts_nop 0\n\t" opa " %0, %0, %0 " WFA_DPP_CTL_MIR "\n\ts_mov_b64 exec, %1"       \
        : "+v"(a), "=&s"(sv)                                                                                        \
        : "s"(wm)                                                                                                   \
        : "scc");
    static WFA_DEV void min_max_min(int &a, int &b, int &c, unsigned long long wm) { WFA_DUO_3("v_min_i32_dpp", "v_max_i32_dpp", "v_min_i32_dpp") }
    static WFA_DEV void min_max(int &a, int &b, unsigned long long wm) { WFA_DUO_2("v_min_i32_dpp", "v_max_i32_dpp") }
    static WFA_DEV void max_add(int &a, int &b, unsigned long long wm) { WFA_DUO_2("v_max_i32_dpp", "v_add_u32_dpp") }
    static WFA_DEV int  max1(int a, unsigned long long wm) {
        WFA_DUO_1("v_max_i32_dpp")
        return a;
    }
    static WFA_DEV int or1(int a, unsigned long long wm) {
        WFA_DUO_1("v_or_b32_dpp")
        return a;
    }
#undef WFA_DUO_3
#undef WFA_DUO_2
#undef WFA_DUO_1
};

// The lanes in which a compare holds, as a mask for the scalar unit (WFA_DUO_UNIFORM, wfa_duo_cfg.hpp).  b must be ONE compare, made where the
// mask is asked for: the ballot of a compare is that compare's own result and costs nothing, but the ballot of anything else -- an AND or an OR
// of compares, a compare made in an earlier block, a stored flag -- is v_cndmask 0 / 1 of the lane mask and a v_cmp with zero of that register:
// two vector instructions to copy a mask that already sits in scalar registers.  `__ballot(run && x) != 0ull` is lowered like that; here the
// masks are combined and tested by the scalar unit instead (s_and_b64, s_cmp_lg_u64), as WF_EXTEND's candidate masks are.  The empty asm keeps
// the compiler from folding mask and test back into a branch on the lane value.
static WFA_DEV unsigned long long duo_lanes(bool b) {
    unsigned long long mask = __builtin_amdgcn_ballot_w64(b);
    asm("" : "+s"(mask));
    return mask;
}
static WFA_DEV bool duo_lane_of(unsigned long long mask) { return __builtin_amdgcn_inverse_ballot_w64(mask); }  // the lane's bit: no instruction

// The kernel's arguments, read again where cold code needs them (WFA_DUO_SCALAR, wfa_duo_cfg.hpp).  KParams is the kernel's one argument, so it
// lies at the start of the kernel-argument segment; a field read through this pointer is a scalar load from constant memory.  The empty asm makes
// the address opaque at the place of the call: the load cannot be hoisted out of the cold block that asks for it, and the field takes no scalar
// register while the score steps run.
template <bool ON>
static WFA_DEV uint32_t duo_uniform(uint32_t x) {
    if constexpr (ON) return (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
    else return x;
}
using DuoArgs = const __attribute__((address_space(4))) KParams;
static WFA_DEV DuoArgs *duo_cold_args() {
    DuoArgs *p = (DuoArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}

// DX / DOE: the penalty shape, as in wfa_blk_kernel (R = max(DX, DOE) rows in the M ring)
// PK: the rings as 16-bit pairs -- a lane's diagonals (p0, p1) in one register and (p2, p3) in another, the lower diagonal in the
// low half -- and WF_NEXT's rejection-free path two diagonals per instruction (wide_next2()); wfa_duo_kernel runs this form.
// PK = false (wfa_duo32_kernel) keeps one 32-bit register per diagonal: the reference the packed form is tested against, word for word.
template <bool CENSUS, int DX, int DOE, bool PK>
__device__ __attribute__((always_inline)) inline void duo_run(const KParams &P) {
    constexpr int PP = 4;
    static_assert(DX >= 1 && DOE >= 1 && DX <= 4 && DOE <= 4, "ring depths of one to four score steps");
    constexpr int R  = DX > DOE ? DX : DOE;
    constexpr int RW = PK ? 2 : PP;  // ring registers per row of a lane
    // the uniform tests as scalar code and the lane constants of set_derived() (wfa_duo_cfg.hpp).  The packed kernel only: the 32-bit-ring
    // reference with three ring rows needs two more scalar registers in this form, and stays as it was
    constexpr bool UNI = WFA_DUO_UNIFORM != 0 && PK;
    // wave-uniform state and cold arguments off the step's path (wfa_duo_cfg.hpp): the packed kernel in its uniform form only
    constexpr int  SCA = WFA_DUO_SCALAR != 0 && UNI ? WFA_DUO_SCALAR_ITEMS : 0;
    constexpr bool SC_ARGS = (SCA & 1) != 0, SC_UNI = (SCA & 2) != 0, SC_SLOW = (SCA & 4) != 0, SC_NZ = (SCA & 8) != 0, SC_SI = (SCA & 16) != 0;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int  lane = threadIdx.x, l7 = lane & 7, l15 = lane & 15;
    const bool hi_half = (lane & 8) != 0;

    const uint32_t  SW = P.lds_seq_words, PW = P.prepack_words;  // PW = 4 + 2 SW words per prepacked pair (a multiple of 4)
    const uint32_t  FP = duo_fetch_pairs(PW), NBUF = duo_bufs(PW);  // pairs per fetch, sequence buffers of the wave
    uint32_t *const park0 = lds + NBUF * PW;
    const uint64_t  cap      = P.arena_words;
    const int       mdd      = (int)P.max_dist_diff;
    const int       minwf    = (int)P.min_wf_len;
    const bool      adaptive = P.adaptive != 0;
    const uint32_t  seed_si  = P.dx;  // the mismatch seed M[x][0] belongs to step x/g
    uint32_t        pk_one   = 0x00010001u;  // (1, 1) for wide_next2()
    if constexpr (PK) asm volatile("" : "+s"(pk_one));
    const int       rows_cap = (int)(cap / 32);  // 16-bit words: a score's 64 diagonals are 32 words

    // ---- per-pair state (identical in the lanes of a pair)
    int       st = 0;  // 0 = free half, 1 = running
    bool      wide = false;
    uint32_t  pidx = 0, si = 0, cells = 0, sbuf = 0;
    int       n = 0, m = 0, kb = 0;
    bool      slow = false, first_eq = false;
    // ---- UNI: the lanes with st == 1 and the lanes with `wide`, as masks in scalar registers: st and wide change in a restructuring round, in fill() and
    // in the finish branch, nowhere else, and each of those ends in set_derived(), which forms the masks again.  The step and the round's trigger
    // read the masks -- `run &&` is a scalar AND, the free halves are ~run_m, DuoRed's fourth stage takes wide_m as it is -- and compare neither
    // st nor wide again.  Between a change and its set_derived() the lane values are the truth, and the code there reads those.
    unsigned long long run_m = 0ull, wide_m = 0ull;
    // (SCA: and the lanes with `slow`.  Written by set_derived() like the other two, and by the step's rare branch that sets the flag; the lane value
    // stays the truth for the park records and for the lanes that join a widening neighbour)
    unsigned long long slow_m = 0ull;
    // ---- per-lane values derived from them
    int             j = l7, k0 = 0;
    // (UNI: what the step would otherwise form again every time, kept in registers -- the kernel has sixteen to spare under the 128 of four waves per
    // SIMD: the window-relative indices 4 j + p and the diagonals k0 + p of the lane's cells, and the upper edge of the window, kb + Wc - 1,
    // that the restructuring trigger compares with.  Written by set_derived() and by nothing else; read through jx(), kx() and kedge)
    int             jp[4] = {4 * l7, 4 * l7 + 1, 4 * l7 + 2, 4 * l7 + 3}, kp[4] = {0, 1, 2, 3}, kedge = 31;
    uint32_t        mdn = 0u, mup = 0u;  // all-ones unless the lane is the first / last of its group
    const uint32_t *lq = lds + 4, *lt = lds + 4;
    uint32_t       *rowp = nullptr;

    uint32_t M[R][RW], I[RW], D[RW];  // offsets, 0 = absent; M[i mod R] = row of step i (PK: two diagonals per register)
    int      rlo[R], rhi[R];          // band of each kept M row (absolute k); empty = (BIG, -BIG)
    int      lim[PP], lmx[PP];
#pragma unroll
    for (int d = 0; d < R; d++) {
        rlo[d] = BK_BIG, rhi[d] = -BK_BIG;
#pragma unroll
        for (int p = 0; p < RW; p++) M[d][p] = 0u;
    }
#pragma unroll
    for (int p = 0; p < RW; p++) I[p] = D[p] = 0u;
#pragma unroll
    for (int p = 0; p < PP; p++) lim[p] = 0, lmx[p] = 0;

    // ---- wave-uniform state
    uint32_t buf_free  = (1u << NBUF) - 1u;      // sequence buffers nobody owns
    uint32_t park_used = 0u;                     // park records in use
    // prefetch pipeline (stages overlap: one new pair per iteration in steady state, three iterations of latency)
    // (one word of flags, not four bools: hipcc merges the stores to two bools into one store through a selected address,
    // which pins both in scratch memory -- two scratch loads per score step)
    constexpr uint32_t PF_TOK = 1u, PF_LD = 2u, PF_STAGED = 4u, PF_DRY = 8u;  // queue atomic in flight / slot loads in flight / a pair staged in LDS / queue exhausted
    // Queue claims.  One returning atomic per fetch on the ONE head word is a ceiling of its own: the word serves about 88 claims
    // a microsecond whatever the waves do in between (KERNELS.md 4a, "Queue claims"), and 1e6 pairs of 1 kbp are 1e6 fetches.
    // So a wave claims BLOCKS of fetches: [pf_next, pf_end) are the entries it has claimed and not fetched yet, and only an empty
    // range costs an atomic.
    //   * the first block needs none: wave w owns [8 w, 8 w + 8) -- a pair per half row; the launch's grid is at most
    //     ceil(chunk_n / 8) waves, so these blocks are disjoint and cover a prefix -- and the head word, which the host zeroes,
    //     hands out the entries from 8 * gridDim.x on (claim_base());
    //   * a claim is B fetches, B = clamp((chunk_n - pf_next) / (2 * gridDim.x * FP), 1, duo_claim) with pf_next the end of the
    //     wave's last range: guided, so that near the queue's end every claim is one fetch and the launch's tail is what it was
    //     (a fixed B would leave one wave with up to B - 1 unstarted fetches while the others leave);
    //   * duo_claim = 1 (debug option): no first block, one fetch per atomic from entry 0 on -- the claiming before blocks.
    // The head word cannot wrap: a wave stops claiming at the first token at or past chunk_n, so the word ends at most
    // gridDim.x * duo_claim * FP <= 4 096 * 8 * 8 entries past chunk_n, and a chunk's pairs own an arena of at least 4 KB each
    // inside a third of the device's memory -- tens of millions of pairs, not 2^32.
    // duo_claim and gridDim.x ride in the spare bits of the flags word (PF_CLAIM_SHIFT, PF_GRID_SHIFT; wfa_host.hip keeps the grid
    // under 65 536): the kernel runs at the limit of its scalar registers, and as two more loop invariants they pushed a mask of the
    // score step out to a vector register's lanes -- two v_readlane a step.  They are read where a wave claims, nowhere else.
    constexpr uint32_t PF_CLAIM_SHIFT = 8u, PF_GRID_SHIFT = 16u;
    uint32_t pf = (umax2(1u, umin2(P.duo_claim, (uint32_t)DUO_CLAIM_MAX)) << PF_CLAIM_SHIFT) | (gridDim.x << PF_GRID_SHIFT);
    uint32_t pf_tok = 0u, pf_ld_idx = 0u, pf_idx = 0u, pf_buf = 0u;
    uint32_t st_mask = 0u;  // buffers of the staged pairs, lowest bit = next pair (queue entry pf_idx)
    uint32_t pf_next = P.duo_claim > 1u ? blockIdx.x * 8u : 0u;
    uint32_t pf_end  = P.duo_claim > 1u ? umin2(pf_next + 8u, P.chunk_n) : 0u;
    const auto claim_base = [&]() { return ((pf >> PF_CLAIM_SHIFT) & 15u) > 1u ? (pf >> PF_GRID_SHIFT) * 8u : 0u; };
    const auto claim_fetches = [&](uint32_t chunk_n) {
        const uint32_t rem = chunk_n > pf_next ? chunk_n - pf_next : 0u;
        return umax2(1u, umin2((pf >> PF_CLAIM_SHIFT) & 15u, rem / (2u * (pf >> PF_GRID_SHIFT) * FP)));
    };
    uint4    pf_w = make_uint4(0u, 0u, 0u, 0u);  // (a slot is at most 256 words: one 16-byte load per lane)

#ifdef WFA_STAMPS  // diagnostic build (scripts/stamps.sh): time per phase and event counts, summed over the waves
    unsigned long long stamp_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, stamp_prev;
    unsigned long long evt[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // wave-steps, restructuring rounds, rounds that move rings, parks,
                                                            // resumes, pairs started, running half-rows, pairs handed on; 8..10: wave-steps that enter
                                                            // WF_EXTEND's continuation, its outer rounds (a candidate per lane), its inner rounds (windows)
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp_prev)::"memory");
#endif
    // The arguments that only cold code reads -- arena, pair_meta, the redo list, work, chunk_first, queue_head, chunk_n, prepack, g, census --
    // SCA: from the kernel-argument segment at the point of use, once per pair or less; else from the registers they occupy all along
    const auto args = [&]() {
        if constexpr (SC_ARGS) return duo_cold_args();
        else return &P;
    };
    const auto pair_of = [&](const auto *A, uint32_t idx) { return A->work ? A->work[idx] : A->chunk_first + idx; };
    const auto redo = [&](const auto *A, uint32_t pair, uint32_t status) {  // (push_redo(), wfa_device.hpp)
        const uint32_t i = atomicAdd(A->redo_count, 1u);
        A->redo_list[2u * i]      = pair;
        A->redo_list[2u * i + 1u] = status;
    };
    // SCA: a wave-uniform value said to be so where it is written (fill(), the evict loop, the hand-on branch, the prefetch stages, the finish:
    // all cold or once per fetch), not at the head of every refill()
    const auto uni = [](uint32_t x) __attribute__((always_inline)) { return duo_uniform<SC_UNI>(x); };
    const auto dn1 = [&](uint32_t x) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, true) & mdn; };
    const auto up1 = [&](uint32_t x) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x101, 0xf, 0xf, true) & mup; };
    const auto other_half = [&](int x) { return __builtin_amdgcn_update_dpp(0, x, 0x128, 0xf, 0xf, true); };  // row_ror:8
    const auto jx = [&](int p) { return UNI ? jp[p] : PP * j + p; };
    const auto kx = [&](int p) { return UNI && p != 0 ? kp[p] : k0 + p; };
    const auto set_derived = [&]() {
        if constexpr (UNI) run_m = duo_lanes(st == 1), wide_m = duo_lanes(wide);
        if constexpr (SC_SLOW) slow_m = duo_lanes(slow);
        const auto *const A = args();
        const uint64_t acap = A->arena_words;
        j   = wide ? l15 : l7;
        mdn = j == 0 ? 0u : ~0u;
        mup = j == (wide ? 15 : 7) ? 0u : ~0u;
        k0  = kb + PP * j;
#pragma unroll
        for (int p = 0; p < PP; p++) lim[p] = imax2(1, imin2(n + k0 + p, m)), lmx[p] = imax2(n + k0 + p, m);
        if constexpr (UNI) {
            static_assert(PP == 4, "four cells a lane");
#pragma unroll
            for (int p = 0; p < PP; p++) {
                jp[p] = PP * j + p, kp[p] = k0 + p;
                // (opaque: knowing how they are formed, the compiler may move the additions back behind the loop's phi, into the step)
                asm("" : "+v"(jp[p]));
                if (p != 0) asm("" : "+v"(kp[p]));
            }
            kedge = kb + (wide ? 64 : 32) - 1;
            asm("" : "+v"(kedge));
        }
        lq   = lds + sbuf * PW + 4u;
        lt   = lq + SW;
        if constexpr (DUO_ARENA_FMT == 10u)  // [pair of groups][score / 8][group & 1][score & 7]: the lane's base; the score's part is added at the store
            rowp = A->arena + (uint64_t)pidx * acap + (((uint32_t)k0 & 56u) >> 3) * (uint32_t)(rows_cap * 4) + (((uint32_t)k0 >> 2) & 1u) * 16u;
        else if constexpr (DUO_ARENA_FMT == 9u)  // [group of four diagonals][score]: the lane's group, then 8 bytes per score
            rowp = A->arena + (uint64_t)pidx * acap + (((uint32_t)k0 & 60u) >> 2) * (uint32_t)(rows_cap * 2) + si * 2u;
        else
            rowp = A->arena + (uint64_t)pidx * acap + (uint64_t)(si >> 3) * 256u + (si & 7u) * 2u;
    };
    const auto clear_rings = [&]() {
#pragma unroll
        for (int d = 0; d < R; d++) {
            rlo[d] = BK_BIG, rhi[d] = -BK_BIG;
#pragma unroll
            for (int p = 0; p < RW; p++) M[d][p] = 0u;
        }
#pragma unroll
        for (int p = 0; p < RW; p++) I[p] = D[p] = 0u;
    };
    // OR over the wave of a value that is the same in the eight lanes of a half row
    const auto or_halves = [&](uint32_t v) {
        uint32_t r = 0u;
#pragma unroll
        for (int o = 0; o < 8; o++) r |= (uint32_t)__builtin_amdgcn_readlane((int)v, 8 * o);
        return r;
    };

    // ================================================================ free halves: parked pairs first, then the staged pair
    // ph = the phase of the NEXT score step: a resumed record's row r, its r-th oldest, goes to M[(ph + r) mod R], and M[ph] is the row that
    // step replaces.  Two callers: the finish branch of step(), for the half it has just freed (WFA_DUO_FILL, wfa_duo_cfg.hpp), and a
    // restructuring round of refill() for what the finish could not place.  Wave-uniform throughout -- m_free is a ballot, the masks and
    // flags are scalars, the staged pair's header words come through readfirstlane -- and the caller follows it with set_derived() and
    // the wave's two fences.
    const auto fill = [&](auto ph_c, unsigned long long m_free) __attribute__((always_inline)) {
        constexpr int ph = decltype(ph_c)::value;
        while (m_free != 0ull && (park_used != 0u || (pf & PF_STAGED) != 0u)) {
            const uint32_t oct  = (uint32_t)__builtin_ctzll(m_free) >> 3;  // wave-uniform
            const bool     mine = ((uint32_t)lane >> 3) == oct;
            if (park_used != 0u) {
                const uint32_t rec = (uint32_t)__builtin_ctz(park_used);
                park_used = uni(park_used & (park_used - 1u));
                WFA_EVT(4, 1);
                const uint32_t *const pr = park0 + rec * DUO_PARK_WORDS;
                if (mine) {
                    // (record row r -> M[(ph + r) mod R]: the phase of the resuming wave, not of the one that parked it)
                    const uint4 *const w = reinterpret_cast<const uint4 *>(pr + 12 * l7);
                    const uint4 v0 = w[0], v1 = R > 2 ? w[1] : make_uint4(0u, 0u, 0u, 0u), v2 = w[2];
                    const uint32_t pw[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                    const uint4 *const s4 = reinterpret_cast<const uint4 *>(pr + 96);
                    const uint4 a0 = s4[0], a1 = s4[1], a2 = s4[2], a3 = s4[3];
                    const uint32_t plo[4] = {a2.x, a2.y, a2.z, a2.w}, phi[4] = {a3.x, a3.y, a3.z, a3.w};
#pragma unroll
                    for (int r = 0; r < R; r++) {
                        if constexpr (PK) {
                            M[(ph + r) % R][0] = pw[2 * r], M[(ph + r) % R][1] = pw[2 * r + 1];
                        } else {
                            M[(ph + r) % R][0] = pw[2 * r] & 0xFFFFu, M[(ph + r) % R][1] = pw[2 * r] >> 16;
                            M[(ph + r) % R][2] = pw[2 * r + 1] & 0xFFFFu, M[(ph + r) % R][3] = pw[2 * r + 1] >> 16;
                        }
                        rlo[(ph + r) % R] = (int)plo[r], rhi[(ph + r) % R] = (int)phi[r];
                    }
                    if constexpr (PK) {
                        I[0] = v2.x, I[1] = v2.y, D[0] = v2.z, D[1] = v2.w;
                    } else {
                        I[0] = v2.x & 0xFFFFu, I[1] = v2.x >> 16, I[2] = v2.y & 0xFFFFu, I[3] = v2.y >> 16;
                        D[0] = v2.z & 0xFFFFu, D[1] = v2.z >> 16, D[2] = v2.w & 0xFFFFu, D[3] = v2.w >> 16;
                    }
                    pidx = a0.x, si = a0.y, cells = a0.z, sbuf = a0.w;
                    n = (int)a1.x, m = (int)a1.y, kb = (int)a1.z, slow = (a1.w & 1u) != 0u, first_eq = (a1.w & 2u) != 0u;
                    st = 1, wide = false;
                }
                m_free &= ~(0xFFull << (8 * oct));
                continue;
            }
            // the next staged pair: header {n, m, status, -} + packed words, in the lowest buffer of st_mask
            pf_buf   = (uint32_t)__builtin_ctz(st_mask);
            st_mask = uni(st_mask & (st_mask - 1u));
            const uint32_t this_idx = pf_idx;
            pf_idx = uni(pf_idx + 1u);
            const uint32_t *const hb = lds + pf_buf * PW;
            // (readfirstlane: an LDS load counts as divergent, and a branch on it would turn this wave-uniform loop and
            // every scalar it updates -- the prefetch flags, the buffer masks -- into per-lane values)
            const uint32_t nq = (uint32_t)__builtin_amdgcn_readfirstlane((int)hb[0]), mt = (uint32_t)__builtin_amdgcn_readfirstlane((int)hb[1]);
            const uint32_t status = (uint32_t)__builtin_amdgcn_readfirstlane((int)hb[2]);
            if (st_mask == 0u) pf = uni(pf & ~PF_STAGED);
            if (status != ST_PENDING) {  // empty / too long / does not fit / a byte outside ACGT: no alignment here
                if (lane == 0) {
                    const auto *const A = args();
                    A->pair_meta[this_idx] = make_uint4(status, 0u, 0u, 0u);
                    if (status >= ST_REDO_BYTES) redo(A, pair_of(A, this_idx), status);
                }
                buf_free = uni(buf_free | (1u << pf_buf));
                continue;  // (the half stays free; the next staged pair will take it)
            }
            WFA_EVT(5, 1);
            if (mine) {
                pidx = this_idx, sbuf = pf_buf;
                n = (int)nq, m = (int)mt;
                const int Ak = m - n;
                si = 0, cells = 0, slow = false;
                kb = -16 + PP * imax2(-3, imin2(3, Ak / (2 * PP)));  // k = 0 (the seed) inside, biased towards Ak
                first_eq = ((hb[4] ^ hb[4 + SW]) & 3u) == 0u;  // q[0] == t[0] (wfa.go:155)
                clear_rings();
                st = 1, wide = false;
            }
            m_free &= ~(0xFFull << (8 * oct));
        }
    };

    // ================================================================ between two score steps
    // prefetch pipeline, then -- only when something has to change -- recentre / widen / narrow / park / resume / start
    const auto refill = [&](auto ph_c) __attribute__((always_inline)) -> bool {
        constexpr int ph  = decltype(ph_c)::value;
        constexpr int NEW = (ph + R - 1) % R;  // ring slot of the newest row; M[ph] is the oldest (replaced by the next step)
        // ---------------------------------------------------------------- prefetch of the next pair, one stage per call
        // (wave-uniform by construction; said so explicitly, or hipcc keeps them in vector registers)
        if constexpr (!SC_UNI) {
            pf        = (uint32_t)__builtin_amdgcn_readfirstlane((int)pf);
            park_used = (uint32_t)__builtin_amdgcn_readfirstlane((int)park_used);
            buf_free  = (uint32_t)__builtin_amdgcn_readfirstlane((int)buf_free);
            st_mask   = (uint32_t)__builtin_amdgcn_readfirstlane((int)st_mask);
            pf_next   = (uint32_t)__builtin_amdgcn_readfirstlane((int)pf_next);
            pf_end    = (uint32_t)__builtin_amdgcn_readfirstlane((int)pf_end);
        }
        if ((pf & (PF_LD | PF_STAGED)) == PF_LD) {  // the words loaded an iteration ago go to spare LDS buffers, one per pair
            // pairs this fetch really holds: the stage below moved pf_next past them an iteration ago, and nothing has moved it since
            const uint32_t cnt = pf_next - pf_ld_idx;
            // the cnt lowest free buffers: slot s of the fetch goes to the s-th of them
            st_mask = 0u;
            {
                uint32_t f = buf_free;
                for (uint32_t c = 0; c < cnt; c++) st_mask |= f & (0u - f), f &= f - 1u;
            }
            st_mask = uni(st_mask), buf_free = uni(buf_free & ~st_mask);
            const uint32_t w0 = (uint32_t)lane * 4u, slot = w0 / PW;  // (a slot is a whole number of 16-byte pieces)
            if (slot < cnt) {
                uint32_t f = st_mask;
                for (uint32_t c = 0; c < slot; c++) f &= f - 1u;
                const uint32_t b = (uint32_t)__builtin_ctz(f);
                *reinterpret_cast<uint4 *>(lds + b * PW + (w0 - slot * PW)) = pf_w;
            }
            pf_idx = uni(pf_ld_idx), pf = uni((pf | PF_STAGED) & ~PF_LD);
        }
        if ((pf & (PF_TOK | PF_LD)) == PF_TOK) {  // the queue entry claimed an iteration ago: its slot's words into registers
            const auto *const A = args();
            if (pf_next >= pf_end) {  // (the wave's range was empty: the token is an atomic's result, the start of a new range)
                const uint32_t chunk_n = A->chunk_n;
                const uint32_t tok = (uint32_t)__builtin_amdgcn_readfirstlane((int)pf_tok) + claim_base();
                const uint32_t blk = claim_fetches(chunk_n) * FP;  // (what the atomic added: pf_next has not moved since)
                pf_next = tok, pf_end = uni(tok < chunk_n ? umin2(tok + blk, chunk_n) : tok);
            }
            pf_ld_idx = uni(pf_next);
            const bool have = pf_next < pf_end;  // (an empty range: the token was at or past chunk_n)
            if (have) {
                const uint32_t *const slot = A->prepack + (uint64_t)pf_ld_idx * PW;
                const uint32_t cnt = umin2(FP, pf_end - pf_next);  // (the last fetch of a range or of the chunk may be partial)
                pf_next += cnt;
                if ((uint32_t)lane * 4u < cnt * PW) pf_w = *reinterpret_cast<const uint4 *>(slot + lane * 4);
            }
            pf_next = uni(pf_next);
            pf = uni((pf & ~PF_TOK) | (have ? PF_LD : PF_DRY));
        }
        if ((pf & (PF_TOK | PF_DRY)) == 0u) {
            // The next fetch: from the wave's range when it has entries left -- no memory operation, the token is pf_next -- else
            // claim_fetches() * FP queue entries, by lane 0, result NOT awaited here: the library is built with
            // -mllvm -amdgpu-atomic-optimizer-strategy=None (Makefile).  With LLVM's atomic optimizer on, this atomicAdd()
            // becomes a wave-aggregated atomic followed AT ONCE by s_waitcnt + v_readfirstlane -- a memory round trip during
            // which the wave's pairs stand still, every four steps; without it the wait sits where the token is read, a
            // score step later.  (An earlier form issued the atomic as inline assembly: same timing, but the compiler then
            // does not know the result is outstanding, and a register copy or a spill of it before the wait would read
            // garbage.  Correct either way with this form; the flag only buys the overlap.)
            if (pf_next >= pf_end) {
                const auto *const A = args();
                const uint32_t blk = claim_fetches(A->chunk_n) * FP;
                if (lane == 0) pf_tok = atomicAdd(A->queue_head, blk);
            }
            pf = uni(pf | PF_TOK);
        }
        // ---------------------------------------------------------------- does anything have to change?
        // (a loop: a parked pair that had asked to widen itself asks again as soon as it has resumed, before it steps)
        unsigned long long m_free;
        WFA_STAMP(0);  // prefetch stage
        for (;;) {
        const int  Wc    = wide ? 64 : 32;
        const bool run   = UNI ? duo_lane_of(run_m) : st == 1;
        bool       touch, narrowable = false;
        unsigned long long m_ev;
        if constexpr (UNI) {
            // (every compare's lane mask on its own, combined by the scalar unit -- duo_lanes(); the window's upper edge from set_derived())
            const unsigned long long touch_m =
                run_m & duo_lanes(rhi[NEW] >= rlo[NEW]) & (duo_lanes(rlo[NEW] <= kb) | duo_lanes(rhi[NEW] >= kedge));
            unsigned long long narrow_m = 0ull;
            if constexpr (ph == 0) {  // (looked at every fourth step: a wide pair that could be narrow costs a half row, nothing else)
                int ulo = rlo[0], uhi = rhi[0];
#pragma unroll
                for (int d = 1; d < R; d++) ulo = imin2(ulo, rlo[d]), uhi = imax2(uhi, rhi[d]);
                narrow_m = run_m & wide_m & duo_lanes(uhi - ulo + 1 <= DUO_NARROW_AT);
            }
            touch = duo_lane_of(touch_m), narrowable = duo_lane_of(narrow_m);
            m_ev = touch_m | narrow_m, m_free = ~run_m;
        } else {
            touch = run && rhi[NEW] >= rlo[NEW] && (rlo[NEW] <= kb || rhi[NEW] >= kb + Wc - 1);
            if constexpr (ph == 0) {  // (looked at every fourth step: a wide pair that could be narrow costs a half row, nothing else)
                int ulo = rlo[0], uhi = rhi[0];
#pragma unroll
                for (int d = 1; d < R; d++) ulo = imin2(ulo, rlo[d]), uhi = imax2(uhi, rhi[d]);
                narrowable    = run && wide && uhi - ulo + 1 <= DUO_NARROW_AT;
            }
            m_ev = __ballot(touch || narrowable), m_free = __ballot(st == 0);
        }
        // (expected: nothing to do -- tells the register allocator that what follows is the cold side of the loop)
        if (__builtin_expect(!(m_ev != 0ull || (m_free != 0ull && (park_used != 0u || (pf & PF_STAGED) != 0u))), 1)) break;
        WFA_EVT(1, 1);
        {
            // ------------------------------------------------------------ what each pair wants
            int ulo = rlo[0], uhi = rhi[0];
#pragma unroll
            for (int d = 1; d < R; d++) ulo = imin2(ulo, rlo[d]), uhi = imax2(uhi, rhi[d]);
            const int span = uhi - ulo + 1;
            int act = 0;  // 1 recentre, 2 widen, 3 narrow, 4 hand on (band wider than a whole row holds)
            if (touch) act = wide ? (span > DUO_WIDE_MAX ? 4 : 1) : (span > DUO_WIDEN_AT ? 2 : 1);
            else if (narrowable) act = 3;
            const int Wn  = act == 2 ? 64 : (act == 3 ? 32 : Wc);
            const int kbn = (((ulo + uhi + 1 - Wn) >> 1) + 2) & ~3;  // the band in the middle of the new window, base a multiple of 4
            // (cannot happen below the thresholds; if it ever did, the pair is handed on -- kbn was computed for Wn, so no other
            // move may be made of this request)
            if (act != 0 && act != 4 && !(ulo - kbn >= 1 && uhi - kbn <= Wn - 2)) act = 4;
            // ------------------------------------------------------------ widening: who takes whose half
            const int  o_act = other_half(act), o_kb = other_half(kb), o_kbn = other_half(kbn);
            const bool o_wide = other_half(wide ? 1 : 0) != 0;
            // both halves of a row ask: the lower one wins, the upper one is parked and asks again when it resumes
            bool widen  = act == 2 && !(hi_half && o_act == 2);
            bool taken  = !wide && !o_wide && o_act == 2 && !(!hi_half && act == 2);  // my half goes to the pair of the other half
            bool evict  = taken && st == 1;
            // ------------------------------------------------------------ park the evicted pairs (LDS records of the wave)
            unsigned long long m_evict = __ballot(evict);
            bool               lost    = false;  // a widening pair whose neighbour cannot be parked: it is handed on instead
            while (m_evict != 0ull) {
                const int      l0   = __builtin_ctzll(m_evict);  // first lane of an evicted half (wave-uniform)
                const uint32_t oct  = (uint32_t)l0 >> 3;
                m_evict &= ~(0xFFull << (8 * oct));
                const bool mine = evict && ((uint32_t)lane >> 3) == oct;
                if (park_used == (1u << DUO_PARK) - 1u) {  // no record left
                    if (((uint32_t)lane >> 3) == (oct ^ 1u)) lost = true;
                    if (mine) evict = false, taken = false;
                    continue;
                }
                const uint32_t rec = (uint32_t)__builtin_ctz(~park_used);
                park_used = uni(park_used | (1u << rec));
                WFA_EVT(3, 1);
                uint32_t *const pr = park0 + rec * DUO_PARK_WORDS;
                if (mine) {
                    // (record row r = the r-th oldest row of the ring, M[(ph + r) mod R]; a ring of fewer than four rows leaves the rest empty)
                    uint4 *const w = reinterpret_cast<uint4 *>(pr + 12 * l7);
                    // (PK: the rings are already the record's 16-bit pairs -- a plain copy)
                    const auto pk  = [](uint32_t lo, uint32_t hi) { return lo | (hi << 16); };
                    const auto pk2 = [&](const uint32_t(&v)[RW], int h) -> uint32_t {
                        if constexpr (PK) return v[h];
                        else return pk(v[2 * h], v[2 * h + 1]);
                    };
                    uint32_t pw[8];
                    int      plo[4], phi[4];
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        pw[2 * r]     = r < R ? pk2(M[(ph + r) % R], 0) : 0u;
                        pw[2 * r + 1] = r < R ? pk2(M[(ph + r) % R], 1) : 0u;
                        plo[r] = r < R ? rlo[(ph + r) % R] : BK_BIG, phi[r] = r < R ? rhi[(ph + r) % R] : -BK_BIG;
                    }
                    w[0] = make_uint4(pw[0], pw[1], pw[2], pw[3]);
                    if constexpr (R > 2) w[1] = make_uint4(pw[4], pw[5], pw[6], pw[7]);
                    w[2] = make_uint4(pk2(I, 0), pk2(I, 1), pk2(D, 0), pk2(D, 1));
                    if (l7 == 0) {
                        uint4 *const s4 = reinterpret_cast<uint4 *>(pr + 96);
                        s4[0] = make_uint4(pidx, si, cells, sbuf);
                        s4[1] = make_uint4((uint32_t)n, (uint32_t)m, (uint32_t)kb, (slow ? 1u : 0u) | (first_eq ? 2u : 0u));
                        s4[2] = make_uint4((uint32_t)plo[0], (uint32_t)plo[1], (uint32_t)plo[2], (uint32_t)plo[3]);
                        s4[3] = make_uint4((uint32_t)phi[0], (uint32_t)phi[1], (uint32_t)phi[2], (uint32_t)phi[3]);
                    }
                }
            }
            if (lost) widen = false, act = 4;
            // a winner that was told "lost" leaves its neighbour alone; the neighbour's lanes must not join it
            {
                const bool o_lost = other_half(lost ? 1 : 0) != 0;
                if (o_lost) taken = false;
            }
            // ------------------------------------------------------------ pairs that are handed on
            if (__ballot(act == 4) != 0ull) {
                WFA_EVT(7, __builtin_popcountll(__ballot(act == 4 && j == 0)));
                if (act == 4 && j == 0) {
                    const auto *const A = args();
                    A->pair_meta[pidx] = make_uint4(ST_REDO_BAND, 0u, 0u, 0u);
                    redo(A, pair_of(A, pidx), ST_REDO_BAND);
                }
                buf_free = uni(or_halves(act == 4 ? (1u << sbuf) : 0u) | buf_free);
                if (act == 4) {
                    st = 0, wide = false;
                    clear_rings();
                }
            }
            // ------------------------------------------------------------ where every lane's rings come from
            // new group: base lane Bn, lanes Gn; old group of the pair the lane belongs to afterwards: base Bo, lanes Go;
            // lane Bn + jn takes the registers of lane Bo + jn + dl (dl = window move in lanes), zeros outside the old group
            const int  rb   = lane & ~15;
            const bool join = taken;  // (evicted or free half that becomes part of the neighbour's pair)
            int src = lane;  // -1: zeros
            bool moved = false, freed = false;
            {
                if (join) {
                    const int Bo = (lane & ~7) ^ 8, dl = (o_kbn - o_kb) >> 2, jo = (lane - rb) + dl;
                    src = (jo >= 0 && jo < 8) ? Bo + jo : -1, moved = true;
                } else if (act == 1) {
                    const int Bo = wide ? rb : (lane & ~7), Go = wide ? 16 : 8, dl = (kbn - kb) >> 2, jo = (lane - Bo) + dl;
                    src = (jo >= 0 && jo < Go) ? Bo + jo : -1, moved = true;
                } else if (widen) {
                    const int Bo = lane & ~7, dl = (kbn - kb) >> 2, jo = (lane - rb) + dl;
                    src = (jo >= 0 && jo < 8) ? Bo + jo : -1, moved = true;
                } else if (act == 3) {
                    const int dl = (kbn - kb) >> 2, jo = (lane - rb) + dl;
                    if (hi_half) src = -1, freed = true;
                    else src = (jo >= 0 && jo < 16) ? rb + jo : -1;
                    moved = true;
                }
            }
            if (__ballot(moved) != 0ull) {
                WFA_EVT(2, 1);
                const int sl = (src < 0 ? lane : src) << 2;
#pragma unroll
                for (int d = 0; d < R; d++)
#pragma unroll
                    for (int p = 0; p < RW; p++) {
                        const uint32_t v = (uint32_t)__builtin_amdgcn_ds_bpermute(sl, (int)M[d][p]);
                        M[d][p]          = src < 0 ? 0u : v;
                    }
#pragma unroll
                for (int p = 0; p < RW; p++) {
                    const uint32_t v = (uint32_t)__builtin_amdgcn_ds_bpermute(sl, (int)I[p]);
                    const uint32_t u = (uint32_t)__builtin_amdgcn_ds_bpermute(sl, (int)D[p]);
                    I[p] = src < 0 ? 0u : v, D[p] = src < 0 ? 0u : u;
                }
                // lanes that join the neighbour's pair take its scalars
                if (__ballot(join) != 0ull) {
                    const int      o_n = other_half(n), o_m = other_half(m);
                    const uint32_t o_pidx = (uint32_t)other_half((int)pidx), o_si = (uint32_t)other_half((int)si);
                    const uint32_t o_cells = (uint32_t)other_half((int)cells), o_sbuf = (uint32_t)other_half((int)sbuf);
                    const int      o_fl = other_half((slow ? 1 : 0) | (first_eq ? 2 : 0));
                    int o_rlo[R], o_rhi[R];
#pragma unroll
                    for (int d = 0; d < R; d++) o_rlo[d] = other_half(rlo[d]), o_rhi[d] = other_half(rhi[d]);
                    if (join) {
                        n = o_n, m = o_m, pidx = o_pidx, si = o_si, cells = o_cells, sbuf = o_sbuf;
                        slow = (o_fl & 1) != 0, first_eq = (o_fl & 2) != 0;
#pragma unroll
                        for (int d = 0; d < R; d++) rlo[d] = o_rlo[d], rhi[d] = o_rhi[d];
                        st = 1;
                    }
                }
                if (join) kb = o_kbn;
                else if (moved && !freed) kb = kbn;
                if (join || widen) wide = true;
                if (act == 3) wide = false;
                if (freed) {
                    st = 0;
#pragma unroll
                    for (int d = 0; d < R; d++) rlo[d] = BK_BIG, rhi[d] = -BK_BIG;
                }
            }
            // ------------------------------------------------------------ free halves: parked pairs first, then the staged pair
            // (what the finish of the step before could not place -- a second half freed there, a pair staged since, a half freed by
            // a narrowing just now; with WFA_DUO_FILL = 0 every fill)
            fill(ph_c, __ballot(st == 0));
            set_derived();
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        }
        WFA_STAMP(1);  // restructuring
        return m_free == ~0ull && park_used == 0u && (pf & (PF_DRY | PF_LD | PF_STAGED)) == PF_DRY;
    };

    // ================================================================ one score step of every running pair
    const auto step = [&](auto ph_c) __attribute__((always_inline)) {
        constexpr int ph = decltype(ph_c)::value;
        // (UNI: "does any RUNNING lane ..." is the ballot of ONE compare and a scalar AND with the mask of the running lanes -- duo_lanes())
        const bool run = UNI ? duo_lane_of(run_m) : st == 1;
        const auto any_run = [&](bool b) {  // b: ONE compare
            if constexpr (UNI) return (duo_lanes(b) & run_m) != 0ull;
            else return __ballot(run && b) != 0ull;
        };
        const unsigned long long wm = UNI ? wide_m : __ballot(wide);  // lanes of the 16-lane pairs (DuoRed's fourth stage)
        WFA_EVT(0, 1), WFA_EVT(6, __builtin_popcountll(__ballot(run)) / 8);

        uint32_t(&Mo)[RW] = M[(ph + R - DOE) % R];  // M[s-o-e]
        uint32_t(&Mx)[RW] = M[(ph + R - DX) % R];   // M[s-x]
        uint32_t(&Mn)[RW] = M[ph];                  // the slot of the row being computed (the oldest row of the ring)

        // ------------------------------------------------------------ WF_NEXT (wfa.go:549-700)
        // (PK: nI, nD and wd as 16-bit pairs, nM as four 32-bit offsets -- WF_EXTEND, the termination test and the band read it per diagonal)
        uint32_t nM[PP], nI[RW], nD[RW], wd[RW], cc[PP];
        // (PK: the neighbours' registers hold two diagonals; k-1 of the lane's first diagonal is the high half of the lower lane's second
        // register, k+1 of its last the low half of the upper lane's first)
        const uint32_t a_edge = dn1(Mo[RW - 1]), b_edge = dn1(I[RW - 1]);
        const uint32_t c_edge = up1(Mo[0]), d_edge = up1(D[0]);
        const bool     slow_any = SC_SLOW ? (slow_m & run_m) != 0ull : any_run(slow);  // (SCA: the stored flag's mask, no compare of it)
        // the path with rejections near a sequence end: 32-bit sources in, 32-bit cells out
        const auto next_slow = [&](const uint32_t(&Mo4)[PP], const uint32_t(&I4)[PP], const uint32_t(&D4)[PP], const uint32_t(&Mx4)[PP],
                                   uint32_t ae, uint32_t be, uint32_t ce, uint32_t de, uint32_t(&nI4)[PP], uint32_t(&nD4)[PP],
                                   uint32_t(&wd4)[PP]) __attribute__((always_inline)) {
#pragma unroll
            for (int p = 0; p < PP; p++) {
                const int      k  = kx(p);
                const uint32_t a0 = p ? Mo4[p - 1] : ae, b0 = p ? I4[p - 1] : be;
                const uint32_t c0 = p < PP - 1 ? Mo4[p + 1] : ce, d0 = p < PP - 1 ? D4[p + 1] : de;
                const uint32_t x0 = Mx4[p];
                // rejections: > m (not >=) for I and X sources, offset - k > n for D and X sources
                const uint32_t a = (int)a0 > m ? 0u : a0, b = (int)b0 > m ? 0u : b0;
                const uint32_t c = (int)c0 - k > n ? 0u : c0, d = (int)d0 - k > n ? 0u : d0;
                const uint32_t x = ((int)x0 > m || (int)x0 - k > n) ? 0u : x0;
                const uint32_t mi = umax2(a, b), tI = umin2(mi, 1u), Isk = mi + tI;
                const uint32_t Dsk = umax2(c, d), tD = umin2(Dsk, 1u);
                const uint32_t x1  = x + umin2(x, 1u);
                const uint32_t Msk = umax3(Isk, Dsk, x1);
                const bool fromX = x != 0u && Msk == x1;  // wfa.go:657-693
                const bool fromI = !fromX && Msk == Isk;
                // backTrace recomputes the pre-extension offset from the un-rejected sources (wfa.go:766-817)
                const uint32_t mu = umax2(a0, b0), Iu = mu + umin2(mu, 1u), Du = umax2(c0, d0);
                const uint32_t Xu = x0 + umin2(x0, 1u);
                const bool     iext = a < b, dext = c < d;
                const uint32_t o0   = (fromI && iext) ? Iu : ((!fromX && !fromI && dext) ? Du : umax3(Iu, Du, Xu));
                const bool     kin  = k >= -(n - 1) && k <= m - 1;  // wfa.go:562-563
                nM[p] = kin ? Msk : 0u, nI4[p] = kin ? Isk : 0u, nD4[p] = kin ? Dsk : 0u;
                wd4[p] = blk_word(o0, iext, dext, fromX, fromI);
                cc[p]  = (CENSUS && kin) ? tI + tD + umin2(Msk, 1u) : 0u;
            }
        };
        if constexpr (PK) {
            if (__builtin_expect(!slow_any, 1)) {
                // the sources of diagonals (p0, p1) and (p2, p3): k-1 of the M[s-o-e] / I rows, k+1 of the M[s-o-e] / D rows
                const uint32_t a0 = __builtin_amdgcn_alignbit(Mo[0], a_edge, 16), a1 = __builtin_amdgcn_alignbit(Mo[1], Mo[0], 16);
                const uint32_t c1 = __builtin_amdgcn_alignbit(c_edge, Mo[1], 16);
                const uint32_t b0 = __builtin_amdgcn_alignbit(I[0], b_edge, 16), b1 = __builtin_amdgcn_alignbit(I[1], I[0], 16);
                const uint32_t d0 = __builtin_amdgcn_alignbit(D[1], D[0], 16), d1 = __builtin_amdgcn_alignbit(d_edge, D[1], 16);
                uint32_t M2[2];
                wide_next2<true>(wide_pk(a0), wide_pk(b0), wide_pk(a1) /* = (M[k0+1], M[k0+2]) */, wide_pk(d0), wide_pk(Mx[0]), wide_pk(pk_one),
                                  M2[0], nI[0], nD[0], wd[0]);
                wide_next2<true>(wide_pk(a1), wide_pk(b1), wide_pk(c1), wide_pk(d1), wide_pk(Mx[1]), wide_pk(pk_one), M2[1], nI[1], nD[1], wd[1]);
#pragma unroll
                for (int p = 0; p < PP; p++) {
                    const int sh = 16 * (p & 1);
                    nM[p] = (M2[p >> 1] >> sh) & 0xFFFFu;
                    // (an I or D cell exists iff its mi or Dsk source does; Isk = mi + 1)
                    cc[p] = CENSUS ? (((nI[p >> 1] >> sh) & 0xFFFFu) != 0u ? 1u : 0u) + (((nD[p >> 1] >> sh) & 0xFFFFu) != 0u ? 1u : 0u) +
                                         (nM[p] != 0u ? 1u : 0u)
                                   : 0u;
                }
            } else {
                uint32_t Mo4[PP], I4[PP], D4[PP], Mx4[PP], nI4[PP], nD4[PP], wd4[PP];
#pragma unroll
                for (int p = 0; p < PP; p++) {
                    const int sh = 16 * (p & 1);
                    Mo4[p] = (Mo[p >> 1] >> sh) & 0xFFFFu, I4[p] = (I[p >> 1] >> sh) & 0xFFFFu;
                    D4[p] = (D[p >> 1] >> sh) & 0xFFFFu, Mx4[p] = (Mx[p >> 1] >> sh) & 0xFFFFu;
                }
                next_slow(Mo4, I4, D4, Mx4, a_edge >> 16, b_edge >> 16, c_edge & 0xFFFFu, d_edge & 0xFFFFu, nI4, nD4, wd4);
#pragma unroll
                for (int h = 0; h < 2; h++)
                    nI[h] = nI4[2 * h] | (nI4[2 * h + 1] << 16), nD[h] = nD4[2 * h] | (nD4[2 * h + 1] << 16),
                    wd[h] = wd4[2 * h] | (wd4[2 * h + 1] << 16);
            }
        } else if (__builtin_expect(!slow_any, 1)) {
#pragma unroll
            for (int p = 0; p < PP; p++) {
                const uint32_t a = p ? Mo[p - 1] : a_edge, b = p ? I[p - 1] : b_edge;
                const uint32_t c = p < PP - 1 ? Mo[p + 1] : c_edge, d = p < PP - 1 ? D[p + 1] : d_edge;
                const uint32_t x = Mx[p];
                const uint32_t mi = umax2(a, b), Isk = mi + (mi != 0u ? 1u : 0u);  // wfa.go:579-609
                const uint32_t Dsk = umax2(c, d);                                   // wfa.go:614-645
                const uint32_t x1  = x + (x != 0u ? 1u : 0u);
                const uint32_t Msk = umax3(Isk, Dsk, x1);                           // wfa.go:655
                nM[p] = Msk, nI[p] = Isk, nD[p] = Dsk;
                wd[p] = blk_word_asm(Msk, a, b, c, d, x1, umax2(Isk, Dsk), Isk, Dsk);  // wfa.go:590-600,626-636,657-693
                cc[p] = CENSUS ? (mi != 0u ? 1u : 0u) + (Dsk != 0u ? 1u : 0u) + (Msk != 0u ? 1u : 0u) : 0u;
            }
        } else {
            next_slow(Mo, I, D, Mx, a_edge, b_edge, c_edge, d_edge, nI, nD, wd);
        }
        // seeds of initComponents (wfa.go:155-160): M[0][0] = 1/Match or M[x][0] = 1/Mismatch
        if (__builtin_expect(any_run(si <= seed_si), 0)) {  // (ONE compare on the step's path; `want` below is the exact test)
            const bool want = run && ((si == 0u && first_eq) || (si == seed_si && !first_eq));
#pragma unroll
            for (int p = 0; p < PP; p++)
                if (want && kx(p) == 0 && nM[p] == 0u) {
                    const uint32_t sw = first_eq ? BLK_SEED_MATCH : BLK_SEED_MISMATCH;
                    nM[p] = 1u, cc[p] = CENSUS ? 1u : 0u;
                    if constexpr (PK) wd[p >> 1] = (p & 1) ? (wd[p >> 1] & 0xFFFFu) | (sw << 16) : (wd[p >> 1] & 0xFFFF0000u) | sw;
                    else wd[p] = sw;
                }
        }
        // ------------------------------------------------------------ store the row's words (CompactView fmt 7)
        // 16-bit words -- a pre-extension offset below 4 096 and the four decisions: this kernel's reads are under 2 048
        // bases -- in tiles of 8 scores x 64 diagonals (1 KB), inside a tile [diagonal / 4][score & 7][diagonal & 3]: a
        // lane's four diagonals are one 8-byte store, and a 64-byte piece of a line holds 8 scores of 4 diagonals.  Half
        // the bytes of fmt 3 to write here and to fetch in the backtrace's walk (round 3; WRITE_SIZE was 31 GB per
        // 1e6 pairs with 32-bit words).
        // (UNI: read again at the finish -- the mask, not a second compare)
        const unsigned long long room_m = UNI ? run_m & duo_lanes((int)si >= rows_cap) : 0ull;
        const bool no_room = UNI ? duo_lane_of(room_m) : run && (int)si >= rows_cap;
        // (SCA: the lanes whose cell p exists, the four compares WF_EXTEND and the band need anyway, made before the store: "has the lane a cell to
        // store" is their OR on the scalar unit, not an OR of the four offsets and a fifth compare)
        unsigned long long nz_m[PP] = {0ull, 0ull, 0ull, 0ull};
        if constexpr (SC_NZ) {
#pragma unroll
            for (int p = 0; p < PP; p++) nz_m[p] = duo_lanes(nM[p] != 0u);
        }
        {
            uint32_t anyc = 0u;
            if constexpr (!SC_NZ) {
#pragma unroll
                for (int p = 0; p < PP; p++) anyc |= nM[p];
            }
            // (fmt 10: score index si -> word (si & ~7) * 4 + (si & 7) * 2 = 2 (si + (si & ~7)) behind the lane's base)
            const uint32_t row_off = DUO_ARENA_FMT == 10u ? 2u * (si + (si & ~7u)) : DUO_ARENA_FMT == 9u ? 0u : (((uint32_t)k0 & 60u) << 2);
            const bool     stored  = SC_NZ ? duo_lane_of(run_m & ~room_m & (nz_m[0] | nz_m[1] | nz_m[2] | nz_m[3])) : run && !no_room && anyc != 0u;
            if (stored) {
                if constexpr (PK) *reinterpret_cast<uint2 *>(rowp + row_off) = make_uint2(wd[0], wd[1]);
                else *reinterpret_cast<uint2 *>(rowp + row_off) = make_uint2(wd[0] | (wd[1] << 16), wd[2] | (wd[3] << 16));
            }
        }
        WFA_STAMP(2);  // next + store

        // ------------------------------------------------------------ WF_EXTEND (wfa.go:381-458)
        bool nz[PP];  // the cell exists: an extension only adds to an offset, so the test made here holds for the rest of the step
        if constexpr (WFA_DUO_EXTEND == 0) {  // the form before (wfa_duo_cfg.hpp): first 16 bases, then a candidate at a time, 16 bases a round
            uint32_t cmask = 0u;
#pragma unroll
            for (int p = 0; p < PP; p++) {
                const int      h    = (int)nM[p];
                uint32_t       rem;  // max(lim - h, 0): one saturating subtraction
                asm("v_sub_u32_e64 %0, %1, %2 clamp" : "=v"(rem) : "v"(lim[p]), "v"(h));
                const uint32_t room = h ? rem : 0u;
                const int      v    = h - kx(p);
                const uint32_t xr   = SeqView<0>::win16(lq, v) ^ SeqView<0>::win16(lt, h);
                const uint32_t rn   = umin2(ffbl_raw(xr) >> 1, room);
                nM[p] += umin2(rn, 16u);
                if (rn > 16u) cmask |= 1u << p;
            }
            if (__ballot(cmask != 0u) != 0ull) WFA_EVT(8, 1);
            while (__ballot(cmask != 0u) != 0ull) {
                WFA_EVT(9, 1);
                const int psel = (int)ffbl_raw(cmask);
                int       h = 0, lm = 0;
#pragma unroll
                for (int p = 0; p < PP; p++)
                    if (psel == p) h = (int)nM[p], lm = lim[p];
                const int kd = k0 + psel;
                bool      go = cmask != 0u;
                do {
                    WFA_EVT(10, 1);
                    const int      rem = lm - h;
                    const uint32_t xr  = SeqView<0>::win16(lq, h - kd) ^ SeqView<0>::win16(lt, h);
                    const uint32_t cnt = umin2(ffbl_raw(xr) >> 1, (uint32_t)imin2(imax2(rem, 0), 16));
                    h += go ? (int)cnt : 0;
                    go = go && xr == 0u && rem > 16;
                } while (__ballot(go) != 0ull);
#pragma unroll
                for (int p = 0; p < PP; p++)
                    if (psel == p) nM[p] = (uint32_t)h;
                cmask &= cmask - 1u;
            }
#pragma unroll
            for (int p = 0; p < PP; p++) nz[p] = nM[p] != 0u;
        } else {
            // first 16 bases of the lane's four diagonals.  A cell that runs on is a CANDIDATE; the candidates of diagonal p are a lane
            // mask in scalar registers (the compare's own result), and everything that decides -- any candidate left? which one does a
            // lane take? does a lane go on? -- is scalar arithmetic on those masks: no flag register to build, test and clear.
            unsigned long long cm[PP];
#pragma unroll
            for (int p = 0; p < PP; p++) {
                int h = (int)nM[p];
                nz[p] = SC_NZ ? duo_lane_of(nz_m[p]) : h != 0;
                // (hides from the compiler that h is below 65 536: knowing it, it forms the text's word address as shift, mask and add;
                // for a value it knows nothing about as shift and shift-add, as it does for the query's)
                asm("" : "+v"(h));
                uint32_t rem;  // max(lim - h, 0): one saturating subtraction
                asm("v_sub_u32_e64 %0, %1, %2 clamp" : "=v"(rem) : "v"(lim[p]), "v"(h));
                const uint32_t room = nz[p] ? rem : 0u;
                const int      v    = h - kx(p);
                const uint32_t xr   = SeqView<0>::win16(lq, v) ^ SeqView<0>::win16(lt, h);
                const uint32_t rn   = umin2(ffbl_raw(xr) >> 1, room);
                nM[p] = (uint32_t)h + umin2(rn, 16u);
                cm[p] = __builtin_amdgcn_ballot_w64(rn > 16u);  // (room >= 17: at least one base is left after the 16)
            }
            static_assert(PP == 4, "candidate masks of four diagonals");
            unsigned long long pend = cm[0] | cm[1] | cm[2] | cm[3];
            if (pend != 0ull) WFA_EVT(8, 1);
            // continuation: every lane takes its lowest candidate, and the wave runs them together, 32 bases a round
            while (pend != 0ull) {
                WFA_EVT(9, 1);
                const unsigned long long s0 = cm[0], s1 = cm[1] & ~cm[0], s2 = cm[2] & ~(cm[0] | cm[1]), s3 = cm[3] & ~(cm[0] | cm[1] | cm[2]);
                const bool sel[PP] = {__builtin_amdgcn_inverse_ballot_w64(s0), __builtin_amdgcn_inverse_ballot_w64(s1),
                                      __builtin_amdgcn_inverse_ballot_w64(s2), __builtin_amdgcn_inverse_ballot_w64(s3)};
                // a lane without a candidate gets h = lm = 0: nothing left, so it counts nothing and never asks for another round
                uint32_t h  = sel[PP - 1] ? nM[PP - 1] : 0u;
                int      kd = kx(PP - 1);
#pragma unroll
                for (int p = PP - 2; p >= 0; p--) h = sel[p] ? nM[p] : h, kd = sel[p] ? kx(p) : kd;
                // lim[] of that diagonal (a candidate has more than 16 bases left: the lower bound of 1 in lim[] cannot bind)
                const uint32_t lm = __builtin_amdgcn_inverse_ballot_w64(pend) ? (uint32_t)imin2(n + kd, m) : 0u;
                // A round counts min(matching bases, bases left, 32); exactly 32 asks for another round.  A lane that has stopped adds
                // nothing in the rounds the others still need: it stands on a mismatch (the next window counts 0) or on lm (0 left; also
                // after a round that used up exactly 32: one round for nothing, then it stops).  h <= lm throughout.  The windows may read
                // one word past a sequence's pad word -- the other sequence, the next buffer or the park area, all inside the wave's LDS:
                // the count never exceeds the bases left, so none of that can count as a match.
                unsigned long long go;
                do {
                    WFA_EVT(10, 1);
                    const uint2    wq = SeqView<0>::win32(lq, (int)h - kd), wt = SeqView<0>::win32(lt, (int)h);
                    const uint32_t b  = umin2(ffbl_raw(wq.x ^ wt.x), ffbl_raw(wq.y ^ wt.y) | 32u);  // first differing bit of the 64; all ones: none
                    const uint32_t t  = umin2(umin2(b >> 1, lm - h), 32u);
                    h += t;
                    go = __builtin_amdgcn_ballot_w64(t == 32u);
                } while (go != 0ull);
#pragma unroll
                for (int p = 0; p < PP; p++) nM[p] = sel[p] ? h : nM[p];
                cm[0] &= ~s0, cm[1] &= ~s1, cm[2] &= ~s2, cm[3] &= ~s3;
                pend = cm[0] | cm[1] | cm[2] | cm[3];
            }
        }
        WFA_STAMP(3);  // extend

        // ------------------------------------------------------------ ends reached? termination (wfa.go:235-239)
        bool hit[PP], hitl = false;
#pragma unroll
        for (int p = 0; p < PP; p++) hit[p] = nM[p] >= (uint32_t)lim[p], hitl |= hit[p];
        bool       term    = false;
        static_assert(PP == 4, "hit masks of four diagonals");
        // (UNI: the OR of the four compares' masks, in scalar registers; hitl, the same OR as a lane value, is read in the rare branch only)
        const bool hit_any = UNI ? (duo_lanes(hit[0]) | duo_lanes(hit[1]) | duo_lanes(hit[2]) | duo_lanes(hit[3])) != 0ull : __ballot(hitl) != 0ull;
        unsigned long long term_m = 0ull;  // UNI: the lanes of `term`
        bool       ghit    = false;
        if (hit_any) {
            bool tl = false;
#pragma unroll
            for (int p = 0; p < PP; p++) tl |= (kx(p) == m - n && nz[p] && (int)nM[p] >= m);
            const int r = DuoRed::or1((hitl ? 1 : 0) | (tl ? 2 : 0), wm);
            ghit = (r & 1) != 0;
            slow |= ghit;
            if constexpr (SC_SLOW) slow_m |= duo_lanes((r & 1) != 0);
            if constexpr (UNI) term_m = duo_lanes((r & 2) != 0) & run_m, term = duo_lane_of(term_m);
            else term = run && (r & 2) != 0;
        }

        // ------------------------------------------------------------ band of the row + wf-adaptive (wfa.go:461-540)
        int      ilo = 0, ihi = -1;  // band to keep (window-relative)
        bool     anyM = false;
        uint32_t csum = 0u;
        if (__builtin_expect(!hit_any, 1)) {
            // (an absent cell's distance is ABSENT, above every threshold: the tests below need no "exists and")
            constexpr int ABSENT = BK_BIG + 1;
            int glo = BK_BIG, ghi = -BK_BIG, dd[PP];
#pragma unroll
            for (int p = PP - 1; p >= 0; p--) glo = nz[p] ? jx(p) : glo;
#pragma unroll
            for (int p = 0; p < PP; p++) {
                ghi   = nz[p] ? jx(p) : ghi;
                dd[p] = nz[p] ? lmx[p] - (int)nM[p] : ABSENT;
            }
            static_assert(PP == 4, "minimum of four distances");
            int mind = imin2(imin2(dd[0], dd[1]), imin2(dd[2], dd[3]));
            DuoRed::min_max_min(glo, ghi, mind, wm);
            anyM = ghi >= 0;
            const bool want = run && adaptive && anyM && (ghi - glo + 1) >= minwf;
            const int  thr  = want ? mind + mdd : BK_BIG;
            int        first_ok = BK_BIG, last_ok = -BK_BIG;
#pragma unroll
            for (int p = PP - 1; p >= 0; p--) first_ok = dd[p] <= thr ? jx(p) : first_ok;
#pragma unroll
            for (int p = 0; p < PP; p++) last_ok = dd[p] <= thr ? jx(p) : last_ok;
            DuoRed::min_max(first_ok, last_ok, wm);
            ilo = first_ok, ihi = last_ok;
#pragma unroll
            for (int p = 0; p < PP; p++) {  // Delete of wfa.go:526-535: the words never exist
                const int  ix   = jx(p);
                const bool keep = ix >= ilo && ix <= ihi;
                nM[p] = keep ? nM[p] : 0u;
                if constexpr (!PK) nI[p] = keep ? nI[p] : 0u, nD[p] = keep ? nD[p] : 0u;  // (PK: at the ring's entry)
                csum += keep ? cc[p] : 0u;
            }
        } else {
            int glo = BK_BIG, ghi = -BK_BIG;
#pragma unroll
            for (int p = PP - 1; p >= 0; p--) glo = nz[p] ? jx(p) : glo;
#pragma unroll
            for (int p = 0; p < PP; p++) ghi = nz[p] ? jx(p) : ghi;
            DuoRed::min_max(glo, ghi, wm);
            anyM = ghi >= 0;
            ilo = glo, ihi = ghi;
            csum = 0u;
#pragma unroll
            for (int p = 0; p < PP; p++) csum += cc[p];
            const bool want_reduce = run && !term && adaptive && anyM && (ghi - glo + 1) >= minwf;
            if (__ballot(want_reduce) != 0ull) {
                int  dd[PP], mind = BK_BIG, maxd = -BK_BIG;
                bool vd[PP];
#pragma unroll
                for (int p = 0; p < PP; p++) {
                    vd[p] = nz[p] && !hit[p];
                    dd[p] = lmx[p] - (int)nM[p];
                    mind  = vd[p] ? imin2(mind, dd[p]) : mind;
                    maxd  = vd[p] ? imax2(maxd, dd[p]) : maxd;
                }
                DuoRed::min_max(mind, maxd, wm);
                const int  thr   = mind + mdd;
                const bool found = want_reduce && mind != BK_BIG && maxd > thr;  // some distance fails (wfa.go:507)
                if (__ballot(found) != 0ull) {
                    int first_ok = BK_BIG, last_ok = -BK_BIG;
#pragma unroll
                    for (int p = PP - 1; p >= 0; p--) first_ok = (vd[p] && dd[p] <= thr) ? jx(p) : first_ok;
#pragma unroll
                    for (int p = 0; p < PP; p++) last_ok = (vd[p] && dd[p] <= thr) ? jx(p) : last_ok;
                    DuoRed::min_max(first_ok, last_ok, wm);
                    // wfa.go:509-511 (see wfa_blk.hpp: per pair, not per wave)
                    int leadp = -1;
#pragma unroll
                    for (int p = 0; p < PP; p++) leadp = (vd[p] && jx(p) < first_ok) ? jx(p) : leadp;
                    leadp = DuoRed::max1(leadp, wm);
                    const int newlo = ghit ? (leadp >= 0 ? leadp + 1 : glo) : first_ok;
                    if (found) ilo = newlo, ihi = last_ok;  // wfa.go:517-524
                    csum = 0u;
#pragma unroll
                    for (int p = 0; p < PP; p++) {
                        const int  ix   = jx(p);
                        const bool keep = ix >= ilo && ix <= ihi;
                        nM[p] = keep ? nM[p] : 0u;
                        if constexpr (!PK) nI[p] = keep ? nI[p] : 0u, nD[p] = keep ? nD[p] : 0u;
                        csum += keep ? cc[p] : 0u;
                    }
                }
            }
        }

        WFA_STAMP(4);  // ranges + wf-adaptive
        // ------------------------------------------------------------ the row's census and position
        const bool keepl = anyM && ihi >= ilo && !no_room;
        if constexpr (CENSUS) {  // (instrumentation instance only: the pair's total, the same in all its lanes)
            int cs = (int)csum, dummy = 0;
            DuoRed::max_add(dummy, cs, wm);
            cells += keepl ? (uint32_t)cs : 0u;
        }
        if constexpr (DUO_ARENA_FMT != 10u) rowp += 2;
        if constexpr (DUO_ARENA_FMT == 7u) rowp += (((uint32_t)(uintptr_t)rowp & 0x38u) == 0u) ? 240 : 0;  // past the tile's 8th score: next tile

        // ------------------------------------------------------------ the new row enters the rings
        if constexpr (PK) {
            // (every offset below 4 096.  An I or D cell outside the kept band needs no select: nM >= Msk >= Isk, Dsk in a cell that
            // exists, and the band's Delete sets nM to 0 -- the minimum with the kept M offset keeps I and D exactly where M is kept)
#pragma unroll
            for (int h = 0; h < 2; h++) {
                Mn[h] = nM[2 * h] | (nM[2 * h + 1] << 16);
                I[h]  = wide_u32(__builtin_elementwise_min(wide_pk(nI[h]), wide_pk(Mn[h])));
                D[h]  = wide_u32(__builtin_elementwise_min(wide_pk(nD[h]), wide_pk(Mn[h])));
            }
        } else {
#pragma unroll
            for (int p = 0; p < PP; p++) Mn[p] = nM[p], I[p] = nI[p], D[p] = nD[p];
        }
        rlo[ph] = keepl ? kb + ilo : BK_BIG;
        rhi[ph] = keepl ? kb + ihi : -BK_BIG;

        // ------------------------------------------------------------ finish / next score
        const unsigned long long fin_m = term_m | room_m;  // (UNI; both inside run_m)
        const bool fin = UNI ? duo_lane_of(fin_m) : run && (term || no_room);
        // (WFA_DUO_FILL: the score index moves on before the finish, not after it -- a pair that finishes keeps its own for pair_meta, and
        // the set_derived() behind the fill forms the row pointer of arena formats 7 and 9 from the index of the next step)
        if constexpr (WFA_DUO_FILL != 0) {
            if constexpr (SC_SI) {  // (one add with the lanes that move on as its carry-in, not a select of 0 / 1 and an add)
                unsigned long long co;
                asm("v_addc_co_u32_e64 %0, %1, %0, 0, %2" : "+v"(si), "=s"(co) : "s"(run_m & ~fin_m));
            } else if (run && !fin) si += 1u;
        }
        // (WFA_DUO_FILL: the branch now holds the fill, and is marked as the cold side so that the step's own path keeps its layout and its
        // registers -- 0.05 ms of a 14 ms step.  Not on the 32-bit rings: at their 124 .. 128 registers the hint costs wfa_duo32_kernel<false, 2, 4>
        // eight spilled ones)
        constexpr bool cold    = WFA_DUO_FILL != 0 && PK;
        const bool     any_fin = UNI ? fin_m != 0ull : __ballot(fin) != 0ull;
        if (cold ? __builtin_expect(any_fin, 0) : any_fin) {
            const auto *const A = args();
            const int ctot = (CENSUS && A->census) ? (int)cells : 0;
            int hf   = 0;  // extended offset of the end cell M[s][Ak]: where the backtrace starts
#pragma unroll
            for (int p = 0; p < PP; p++)
                if (kx(p) == m - n) hf = (int)nM[p];  // (= the ring's new row)
            hf = DuoRed::max1(hf, wm);
            if (fin && j == 0) {
                if (no_room) {
                    A->pair_meta[pidx] = make_uint4(ST_REDO_ARENA, 0u, 0u, 0u);
                    redo(A, pair_of(A, pidx), ST_REDO_ARENA);
                } else {
                    A->pair_meta[pidx] = make_uint4(ST_OK, si * A->g, (uint32_t)hf, (uint32_t)ctot);
                }
            }
            // (or_halves() first, buf_free second, as `buf_free |= or_halves(..)` reads them: the other order moved the register allocation of the whole
            // loop -- six vector instructions more on the step's path, profiles/r15_duo_scalar.txt)
            buf_free = uni(or_halves(fin ? (1u << sbuf) : 0u) | buf_free);
            if (fin) {
                st = 0, wide = false;
                clear_rings();
            }
            if constexpr (WFA_DUO_FILL != 0) {
                // The freed half takes the next pair here and now -- a parked pair, else the staged one -- instead of asking for a
                // restructuring round that would move nobody's rings (about 0.9 such rounds a pair at 1 kbp, each the price of a score
                // step), and it runs in the very next step.  The rows go where the next step expects them: its phase.  Nothing to place
                // (the queue is dry, the next pair not staged yet): the half waits for a round, as before.
                fill(std::integral_constant<int, (ph + 1) % R>{}, __ballot(st == 0));
                set_derived();
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
        if constexpr (WFA_DUO_FILL == 0) {
            if (run && !fin) si += 1u;
            if constexpr (UNI)
                if (any_fin) set_derived();  // (st and wide of the finished pairs have changed: the masks; nothing else of it differs)
        }
        WFA_STAMP(5);  // ring + finish
    };

    for (;;) {
        if (refill(std::integral_constant<int, 0>{})) break;
        step(std::integral_constant<int, 0>{});
        if constexpr (R > 1) {
            if (refill(std::integral_constant<int, 1 % R>{})) break;
            step(std::integral_constant<int, 1 % R>{});
        }
        if constexpr (R > 2) {
            if (refill(std::integral_constant<int, 2 % R>{})) break;
            step(std::integral_constant<int, 2 % R>{});
        }
        if constexpr (R > 3) {
            if (refill(std::integral_constant<int, 3 % R>{})) break;
            step(std::integral_constant<int, 3 % R>{});
        }
    }
#ifdef WFA_STAMPS
    if (lane == 0 && P.debug_info) {
        unsigned long long *acc = reinterpret_cast<unsigned long long *>(P.debug_info);
        for (int i = 0; i < 8; i++) atomicAdd(acc + i, stamp_acc[i]);
        for (int i = 0; i < 16; i++) atomicAdd(acc + 8 + i, evt[i]);
    }
#endif
}

#ifndef WFA_DUO_VGPRS
#define WFA_DUO_VGPRS 64  // (the attribute counts register PAIRS on gfx90a and later: 64 = no cap below the 128 of four waves per SIMD; 60 = 120 VGPRs)
#endif
// The offsets of a pair fit 16 bits: wfa_duo_kernel only takes pairs whose prepacked slot fits 256 words (4 header words + 2 x 126 words
// of 16 bases), so its reads are under 2 048 bases and every offset under 4 096 -- the 12 bits blk_word() gives it in a halfword.
static_assert(16u * (256u - 4u) / 2u < 2048u, "wfa_duo_kernel's packed rings need offsets under 4 096");
template <bool CENSUS, int DX = 2, int DOE = 4>
__global__ __launch_bounds__(64, WFA_DUO_WAVES) __attribute__((amdgpu_num_vgpr(WFA_DUO_VGPRS))) void wfa_duo_kernel(const KParams P) {
    duo_run<CENSUS, DX, DOE, true>(P);
}
// the 32-bit rings: the reference of the packed kernel (debug option duo_pk = 0)
template <bool CENSUS, int DX = 2, int DOE = 4>
__global__ __launch_bounds__(64, WFA_DUO_WAVES) __attribute__((amdgpu_num_vgpr(WFA_DUO_VGPRS))) void wfa_duo32_kernel(const KParams P) {
    duo_run<CENSUS, DX, DOE, false>(P);
}

}  // namespace wfa
