// wfa_ladder.hpp -- the plan of one job of the long-pair ladder (align_device, wfa_host.hip): which of wfa_generic_kernel,
// wfa_team_kernel and wfa_teamc_kernel the job launches, its arena slots or paged pool, the team geometry and the LDS of the
// launch.  Arithmetic on the device's size, a dozen options, the penalties and the job; it touches no device state.  Host only,
// no HIP includes: tests/ladder_host_test.cpp compiles it stand-alone.  The constants the plan shares with the kernels have their
// one definition here; the kernels' headers include this one.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include "wfa_kinds.hpp"

namespace wfa {

constexpr size_t LDS_MAX_BYTES = 160 * 1024;
constexpr int DIR_ENT_BYTES = 32;                 // sizeof(DirEnt) (wfa_common.hpp)
constexpr int DIR_WORDS     = DIR_ENT_BYTES / 4;
constexpr int GEN_LDS_EXTRA_WORDS = 16;           // wfa_generic_kernel: LDS words used besides the two packed sequences
constexpr int WAVE_DIR_RING = 64;                 // wave mode: directory entries in LDS (sources reach back < 64 scores)
constexpr int TEAM_RING     = WAVE_DIR_RING;      // directory entries every workgroup of a team keeps in LDS
constexpr int TEAM_MAX_PAGES = 1024;              // pages one pair can hold (its list in page_ctl)
#ifndef WFA_TC_THREADS
#define WFA_TC_THREADS 1024
#endif
constexpr int TC_THREADS = WFA_TC_THREADS;        // wfa_teamc_kernel (wfa_teamc.hpp)
constexpr int TC_STRIPE  = 4096;                  // diagonals of a workgroup's stripe
constexpr int TC_U       = TC_STRIPE / TC_THREADS;
constexpr int TC_ROWW    = TC_STRIPE + 2;         // LDS words of a ring row: the stripe and a halo cell at either end
constexpr int TC_RED     = 80;                    // ints of the workgroup's scratch in LDS (red[])
constexpr int TC_MAX_T   = 64;                    // workgroups per team (one lane of the polling wave each)

// What the plan reads: filled from the context, the call's KParams and debug_single in one place (ladder_env, wfa_host.hip).
struct LadderEnv {
    uint64_t total_mem;
    int      num_cus;
    int64_t  arena_budget_pct, arena_bytes_per_slot, slots, threads_per_pair;  // the options of these names (wfa_ctx.hpp)
    int64_t  team_min_len, team_wgs, team_wave, team_compact, team_paged, team_scout, team_xcd;
    bool     debug_single, dbg_teamc;  // the one-pair debug launch; ... of wfahip_debug_team_compact
    uint32_t x, oe, e, g;              // penalties and what they share (KParams)
    bool     global_alignment, adaptive;

    // Bytes of device memory the ladder's arenas may take: 60 % by default -- four 43 GB slots for the hard 100 kbp semi-global
    // pairs (a team of workgroups each).  More slots were measured and lose to the re-runs of the pairs that outgrow them
    // (option arena_budget_pct).
    uint64_t budget_bytes() const { return (uint64_t)((double)total_mem * std::min(0.9, std::max(0.1, (double)arena_budget_pct / 100.0))); }
    // teams are for pairs of at least team_min_len bases
    bool long_pairs(uint32_t max_len) const { return team_min_len > 0 && max_len >= (uint64_t)team_min_len; }
    // score indices the farthest source of a row lies back
    uint32_t reach() const { return std::max(x, std::max(oe, e)) / g; }
};

struct LaunchCfg {
    int      waves = 0;    // 1, 4 or 16 waves per pair
    int      mode  = 0;    // 0 = 2-bit LDS, 1 = bytes in global memory
    uint32_t lds_seq_words = 0;
    size_t   lds_bytes     = 0;
    uint64_t arena_words   = 0;  // per slot; of the whole pool when the launch is paged
    uint32_t slots         = 0;
};

// The slot sizes of the ladder for pairs of up to max_len bases, level by level from level 0.
// x8, x8, then x2 per level -- a slot of a long pair is tens of GB by then, and every doubling halves the number of pairs that
// can be in flight (level 3 of a 100 kbp semi-global pair: 19.7 GB).  Once at most six slots fit the budget, a level is "one
// slot fewer", and a slot takes its whole share of the budget: 5 x 46 GB, 4 x 57, 3 x 76, 2 x 115, 1 x 230 on a 288 GB device
// with the budget at 80 % (60 %: 4 x 43, 3 x 57, 2 x 86, 1 x 172) -- every slot dropped is a team of workgroups less in flight.
// (tests/ladder_host_test.cpp has these figures.)
struct SlotLadder {
    uint64_t budget_words, words;  // the budget; what the next level grows from
    bool     sized;                // option arena_bytes_per_slot: an explicit size never becomes a share of the budget
    int      level = 0;
    SlotLadder(const LadderEnv &E, uint32_t max_len) : budget_words(E.budget_bytes() / 4ull), sized(E.arena_bytes_per_slot > 0) {
        // semi-global rows are n+m-1 wide until wf-adaptive collapses the band (a few dozen scores): ~4x the words
        words = sized ? std::max<uint64_t>(4096, E.arena_bytes_per_slot / 4) : std::max<uint64_t>(64 * 1024, (E.global_alignment ? 96ull : 384ull) * max_len);
    }
    void climb() {
        const uint64_t fit = budget_words / words;
        words = fit >= 2 && fit <= 6 ? budget_words / (fit - 1) : words * (level < 2 ? 8 : 2);
        level++;
    }
    uint64_t slot() const {  // words of a slot at this level
        const uint64_t fit = budget_words / words;
        return (fit >= 1 && fit <= 6 && !sized ? budget_words / fit : words) & ~7ull;  // directory entries are 32-byte aligned from the slot end
    }
};
inline uint64_t ladder_slot_words(const LadderEnv &E, uint32_t max_len, int level) {
    SlotLadder l(E, max_len);
    while (l.level < level) l.climb();
    return l.slot();
}

// Launch configuration of wfa_generic_kernel for one job: CFG_OK, or why there is none.
enum : int { CFG_OK = 0, CFG_LDS = 1 /* the sequences do not fit LDS: mode 1 */, CFG_NO_SLOT = 2 /* not one slot fits the budget */ };
inline int make_cfg(const LadderEnv &E, uint32_t max_len, int mode, int level, uint64_t n_work, LaunchCfg &c) {
    c.waves = max_len <= 4096 ? 1 : (max_len <= 65536 ? 4 : 16);
    if (E.threads_per_pair > 0) c.waves = E.threads_per_pair <= 64 ? 1 : (E.threads_per_pair <= 256 ? 4 : 16);
    c.mode          = mode;
    c.lds_seq_words = (mode == 0) ? ((max_len + 15) / 16 + 1) : 0;
    c.lds_bytes     = (2ull * c.lds_seq_words + GEN_LDS_EXTRA_WORDS) * 4ull;
    if (c.lds_bytes > LDS_MAX_BYTES) return CFG_LDS;
    c.arena_words = ladder_slot_words(E, max_len, level);
    const uint64_t fit = E.budget_bytes() / 4ull / c.arena_words;
    if (fit == 0) return CFG_NO_SLOT;
    // resident workgroups per CU: 32 wave slots, LDS
    const uint32_t per_cu = std::max<uint32_t>(1, std::min<uint32_t>(32 / c.waves, (uint32_t)(LDS_MAX_BYTES / c.lds_bytes)));
    const uint64_t slots  = E.slots > 0 ? (uint64_t)E.slots : (uint64_t)E.num_cus * per_cu;
    c.slots = (uint32_t)std::min(std::min(slots, fit), std::max<uint64_t>(n_work, 1));
    return CFG_OK;
}

// rows of a wave-mode LDS ring: the power of two above the farthest source
inline uint32_t wave_ring_rows(const LadderEnv &E) {
    uint32_t rows = 2;
    while (rows <= E.reach()) rows *= 2;
    return rows;
}
inline size_t wave_ring_bytes(uint32_t rows) { return (size_t)rows * 3 * 64 * 4; }  // M, I and D of 64 diagonals

struct LadderPlan {
    bool      launch = false;  // false: neither a slot nor a pool fits the budget -- the job's pairs end as "no memory"
    int       mode = 0, level = 0;  // as used: after the byte-path fallback and the climb down of a learned start level
    Kind      kind = K_GENERIC;     // the kernel of the launch: K_GENERIC, K_TEAM or K_TEAMC
    LaunchCfg cfg;                  // cfg.lds_bytes: of wfa_generic_kernel / wfa_team_kernel, wave-mode rings included
    uint32_t  team_T = 0, team_n = 0;  // workgroups per team (as the XCD mapping sets it), teams; 0: one workgroup per pair
    uint32_t  team_wave_rows = 0;      // rows of the teams' wave-mode ring, 0 = none
    bool      team_c = false;          // wfa_teamc_kernel's LDS rings fit (kind says whether its team size does too)
    size_t    lds_c  = 0;              // ... and its LDS bytes
    bool      paged = false, scout_now = false;  // one pool of pages for all teams; the scout pass (a team is ONE workgroup)
    uint64_t  pool_words = 0, dir_words = 0;     // the pool; the directory region of a team behind its pages
    uint32_t  page_log = 0, n_pages = 0;
    bool      xmap = false;  // teams of one XCD's CUs (team = blockIdx % 8)
    uint32_t  grid = 0;      // workgroups of a team launch
    uint32_t  wave_bt = 0, wave_rows = 0;  // wfa_generic_kernel's wave mode (KParams of these names)
};

// The plan of a job over n_work pairs of up to max_len bases: starts in `mode` at `level`; hint: the level was learned from an
// earlier call, not reached from a failed level below it; scout: the job may run as the team kernel's scout pass.
inline LadderPlan plan_ladder_job(const LadderEnv &E, int mode, int level, bool hint, bool scout, uint64_t n_work, uint32_t max_len) {
    LadderPlan p;
    LaunchCfg &cfg = p.cfg;
    const uint64_t budget = E.budget_bytes(), budget_w = budget / 4ull;
    const uint32_t cus = (uint32_t)std::max(1, E.num_cus);
    int cr = make_cfg(E, max_len, mode, level, n_work, cfg);
    if (cr == CFG_LDS) cr = make_cfg(E, max_len, mode = 1, level, n_work, cfg);  // byte path for the whole job
    // a learned start level whose slot does not fit (the class buckets lengths by powers of two, slots scale with the
    // length): climb down to the largest level that does, never straight to "no memory"
    while (cr == CFG_NO_SLOT && hint && level > 0) cr = make_cfg(E, max_len, mode, --level, n_work, cfg);
    p.mode = mode, p.level = level;
    // (the paged team kernel has levels beyond "one slot of this level fits": the pool is the whole budget there and a level
    // halves the teams that share it -- the launch configuration is then that of the last level whose slot fitted)
    const bool paged_capable = E.team_paged != 0 && !E.debug_single && E.team_wgs == 0 && E.arena_bytes_per_slot <= 0 && E.long_pairs(max_len) && E.e != 0u;
    const bool no_slot_fits  = cr == CFG_NO_SLOT;  // (if the paged launch does not happen after all, the job ends as "no memory")
    for (int lv = level; cr == CFG_NO_SLOT && paged_capable && lv > 0;) cr = make_cfg(E, max_len, mode, --lv, n_work, cfg);
    if (E.debug_single) cfg.slots = 1;
    // Wide wavefronts: a team of workgroups per pair (wfa_team_kernel) instead of one workgroup per pair.  It pays when one
    // workgroup per pair cannot fill the GPU: few pairs, or arenas so large that only a few fit (cfg.slots is the number of
    // pairs the generic kernel could run at once).
    uint32_t t0 = (uint32_t)std::min<uint64_t>(cus, std::max<uint64_t>(2, (2ull * max_len + 8191) / 8192));
    if (E.team_wgs > 0) t0 = (uint32_t)std::min<int64_t>(cus, E.team_wgs);
    if (cr == CFG_OK && (!E.debug_single || E.team_wgs > 0) && E.long_pairs(max_len) && (cfg.slots < (uint32_t)std::max(1, E.num_cus / 2) || E.team_wgs > 0) &&
        E.e != 0u && E.reach() < (uint32_t)TEAM_RING) {
        p.team_n = (uint32_t)std::min<uint64_t>(n_work, std::max<uint32_t>(1, cus / t0));
        // one arena per team
        while (p.team_n > 1 && (uint64_t)p.team_n * cfg.arena_words * 4ull > budget) p.team_n--;
        if ((uint64_t)p.team_n * cfg.arena_words * 4ull > budget) cr = CFG_NO_SLOT;
        p.team_T          = E.team_wgs > 0 ? t0 : std::min<uint32_t>(cus / p.team_n, 2 * t0);  // ~2 cells per thread and stripe
        cfg.slots         = p.team_n;
        cfg.lds_seq_words = (cfg.lds_seq_words + 1u) & ~1u;
        cfg.lds_bytes     = (2ull * cfg.lds_seq_words + 16 + TEAM_RING * DIR_WORDS) * 4ull;
        if (cfg.lds_bytes > LDS_MAX_BYTES) p.team_T = 0;  // (cannot happen: make_cfg already bounded the sequences)
        // wave mode: an LDS ring of the last rows, if it fits
        const uint32_t rows = wave_ring_rows(E);
        if (E.team_wave && rows <= (uint32_t)TEAM_RING && cfg.lds_bytes + wave_ring_bytes(rows) <= LDS_MAX_BYTES)
            p.team_wave_rows = rows, cfg.lds_bytes += wave_ring_bytes(rows);
    }
    // wfa_teamc_kernel instead of wfa_team_kernel when its LDS rings fit beside the sequences: rows of max(x, o+e)/g + 2 e/g
    // x 4 098 words (the default penalties: six rows, 96 KB; a 100 kbp pair's packed sequences: 50 KB)
    if (p.team_T > 0 && E.team_compact != 0 && (!E.debug_single || E.dbg_teamc) && max_len < (1u << 27)) {
        const uint32_t rm = std::max(E.x, E.oe) / E.g, re = E.e / E.g;
        p.lds_c  = (2ull * cfg.lds_seq_words + TC_RED + TEAM_RING * DIR_WORDS) * 4ull + wave_ring_bytes(p.team_wave_rows) + (size_t)64 * TC_U * 4 +
                   (size_t)(rm + 2 * re) * TC_ROWW * 4;
        p.team_c = p.lds_c <= LDS_MAX_BYTES;
    }
    // Paged arena of the team kernel: ONE pool for all teams, a pair takes pages as its rows grow.  The ladder level sizes the
    // pool (as many slot sizes as there are teams) until that reaches the budget; from there a level halves the number of
    // teams that share it -- down to one team with the whole pool.
    if (p.team_T > 0 && paged_capable) {
        uint32_t teams = (uint32_t)std::min<uint64_t>(n_work, std::max<uint32_t>(1, std::min<uint32_t>(8u, cus / t0)));
        // scout pass (wfa_teamc_kernel only): a team is ONE workgroup, as many teams as CUs; it finishes the pairs whose band
        // collapses and hands the others on.  Worth a launch of its own when the teams would otherwise take several pairs each.
        p.scout_now = scout && p.team_c && E.team_scout != 0 && E.adaptive && (E.team_scout >= 2 || n_work > 2ull * teams);
        const uint32_t teams_full = teams;
        if (p.scout_now) teams = (uint32_t)std::min<uint64_t>(n_work, cus);
        // the levels up to this one at which `teams` slots no longer fit the budget.  over = 1: the first of them -- all teams,
        // the whole budget; every further level halves the teams
        SlotLadder l(E, max_len);
        int        over = (uint64_t)teams * l.slot() > budget_w;
        while (l.level < level) l.climb(), over += (uint64_t)teams * l.slot() > budget_w;
        const bool spent = over > 1 && (teams >> (over - 2)) <= 1u;  // the level before already ran ONE team with the whole pool
        if (over > 1) teams = std::max<uint32_t>(1, teams >> (over - 1));
        // a directory entry per score index up to the worst score two sequences of this length can reach (every base a
        // mismatch or part of one long gap), per team, behind the pages
        const uint64_t worst_idx = ((uint64_t)(E.x + E.e) * max_len + 2ull * E.oe) / E.g + 64;
        p.dir_words = ((uint64_t)DIR_WORDS * worst_idx + 4095) & ~4095ull;
        const uint64_t dirs = (uint64_t)teams * p.dir_words;
        const uint64_t rows_words = over > 0 ? (budget_w > dirs ? budget_w - dirs : 0) : std::min<uint64_t>(budget_w, (uint64_t)teams * l.slot());
        // pages of 1/64 of the rows' share, between "a row and then some" and 256 MB
        uint64_t pw = 1ull << 20;
        while (pw < 8ull * max_len) pw <<= 1;
        while (pw < (64ull << 20) && pw * 64 < rows_words) pw <<= 1;
        while ((1ull << p.page_log) < pw) p.page_log++;
        p.n_pages    = (uint32_t)std::min<uint64_t>(rows_words >> p.page_log, 1u << 20);
        p.pool_words = ((uint64_t)p.n_pages << p.page_log) + dirs;
        if (spent) {
            cr = CFG_NO_SLOT;
        } else if (p.n_pages >= teams) {
            p.paged = true, p.team_n = teams, cr = CFG_OK;
            p.team_T = p.scout_now ? 1u : std::min<uint32_t>(cus / p.team_n, 2 * t0);
        } else if (p.scout_now && p.n_pages >= teams_full) {  // (too few pages for a team per CU: as many scouts as there are pages)
            p.paged = true, p.team_n = std::min<uint32_t>(teams, p.n_pages), cr = CFG_OK;
            p.team_T = 1u;
        }
        if (!p.paged) p.scout_now = false;
        else cfg.slots = p.team_n, cfg.arena_words = p.pool_words;
    }
    if (no_slot_fits && !p.paged) cr = CFG_NO_SLOT;  // (the configuration of a lower level was only borrowed for the paged launch)
    p.launch = cr == CFG_OK;
    if (p.team_T > 0) {
        // teams of one XCD's CUs (team = blockIdx % 8) when at most eight teams run and the CUs divide by eight
        p.xmap = E.team_xcd != 0 && E.team_wgs == 0 && p.team_n <= 8 && E.num_cus % 8 == 0 && E.num_cus >= 16;
        p.grid = p.xmap ? (uint32_t)E.num_cus : p.team_n * p.team_T;
        if (p.xmap) p.team_T = (uint32_t)E.num_cus / 8u;
        p.kind = p.team_c && p.team_T <= (uint32_t)TC_MAX_T ? K_TEAMC : K_TEAM;
    } else if (E.team_wave && E.reach() < (uint32_t)WAVE_DIR_RING) {
        // wave mode of the generic kernel: directory ring + ring of the last rows in LDS, if they fit
        const size_t dir_bytes = 16 + (size_t)WAVE_DIR_RING * DIR_ENT_BYTES, ring_bytes = wave_ring_bytes(wave_ring_rows(E));
        if (cfg.lds_bytes + dir_bytes <= LDS_MAX_BYTES) {
            p.wave_bt = 1, cfg.lds_bytes += dir_bytes;
            if (E.e != 0u && cfg.lds_bytes + ring_bytes <= LDS_MAX_BYTES) p.wave_rows = wave_ring_rows(E), cfg.lds_bytes += ring_bytes;
        }
    }
    return p;
}

}  // namespace wfa
