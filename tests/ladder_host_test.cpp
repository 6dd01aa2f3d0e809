// Stand-alone check of wfa_amd/csrc/wfa_ladder.hpp (host only): the plan of one job of the long-pair ladder -- kernel, arena slots or
// paged pool, team geometry, LDS -- against plans written out as literals, the slot sizes the comments quote, and invariants over a
// grid of devices, options, penalties and jobs.  The literals were taken from the sizing code as it stood inline in align_device
// (wfa_host.hip) before it became plan_ladder_job(); the two agreed on every one of the grid's 650 280 960 cases
// (profiles/r12_ladder_refactor.txt).  Built under the host sanitizers by tests/test_ladder_host.py.
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>
#include "../wfa_amd/csrc/wfa_ladder.hpp"

using namespace wfa;

namespace {

enum { F_LAUNCH, F_MODE, F_LEVEL, F_KIND, F_WAVES, F_CFG_MODE, F_LDS_SEQ_WORDS, F_LDS_BYTES, F_ARENA_WORDS, F_SLOTS, F_TEAM_T, F_TEAM_N, F_TEAM_WAVE_ROWS,
       F_TEAM_C, F_LDS_C, F_PAGED, F_SCOUT_NOW, F_POOL_WORDS, F_DIR_WORDS, F_PAGE_LOG, F_N_PAGES, F_XMAP, F_GRID, F_WAVE_BT, F_WAVE_ROWS, F_COUNT };
const char *const FIELD[F_COUNT] = {"launch", "mode", "level", "kind", "cfg.waves", "cfg.mode", "cfg.lds_seq_words", "cfg.lds_bytes", "cfg.arena_words", "cfg.slots", "team_T", "team_n",
                                    "team_wave_rows", "team_c", "lds_c", "paged", "scout_now", "pool_words", "dir_words", "page_log", "n_pages", "xmap", "grid", "wave_bt", "wave_rows"};

struct JobIn {
    LadderEnv env;  // {total_mem, num_cus, arena_budget_pct, arena_bytes_per_slot, slots, threads_per_pair, team_min_len, team_wgs, team_wave, team_compact,
                    //  team_paged, team_scout, team_xcd, debug_single, dbg_teamc, x, o + e, e, g, global_alignment, adaptive}
    int      mode, level, hint, scout;
    uint64_t n_work;
    uint32_t max_len;
};
struct Row {
    JobIn    in;
    uint64_t want[F_COUNT];  // (a job that does not launch: launch, mode and level only)
};

void flatten(const LadderPlan &p, uint64_t *f) {
    const uint64_t v[F_COUNT] = {p.launch, (uint64_t)p.mode, (uint64_t)p.level, (uint64_t)p.kind, (uint64_t)p.cfg.waves, (uint64_t)p.cfg.mode, p.cfg.lds_seq_words, p.cfg.lds_bytes,
                                 p.cfg.arena_words, p.cfg.slots, p.team_T, p.team_n, p.team_wave_rows, p.team_c, p.lds_c, p.paged, p.scout_now, p.pool_words, p.dir_words,
                                 p.page_log, p.n_pages, p.xmap, p.grid, p.wave_bt, p.wave_rows};
    for (int i = 0; i < F_COUNT; i++) f[i] = v[i];
}
bool same(const uint64_t *a, const uint64_t *b) {
    uint64_t d = 0;
    for (int i = 0; i < F_COUNT; i++) d |= a[i] ^ b[i];
    return d == 0;
}
LadderPlan plan(const JobIn &j) { return plan_ladder_job(j.env, j.mode, j.level, j.hint != 0, j.scout != 0, j.n_work, j.max_len); }

// Defaults of the options, a 288 GB device of 256 CUs, penalties 4/6/2 (x, o + e, e, g = 4, 8, 2, 2), wf-adaptive on, first launch of a call
// (scout 1) unless a row says otherwise.
const Row ROWS[] = {
    // 32 x 100 kbp semi-global, 288 GB, budget 60 %, a slot per team, level 3
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 0, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 3, 0, 1, 32ull, 100000u},
     {1, 0, 3, 17, 16, 0, 6252, 58272, 4915200000ull, 8, 32, 8, 8, 1, 157904, 0, 0, 0, 0, 0, 0, 1, 256, 0, 0}},
    // 32 x 100 kbp semi-global, 288 GB, budget 60 %, a slot per team, level 4
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 0, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 4, 0, 1, 32ull, 100000u},
     {1, 0, 4, 17, 16, 0, 6252, 58272, 10800000000ull, 4, 32, 4, 8, 1, 157904, 0, 0, 0, 0, 0, 0, 1, 256, 0, 0}},
    // 32 x 100 kbp semi-global, 288 GB, budget 60 %, a slot per team, level 5
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 0, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 5, 0, 1, 32ull, 100000u},
     {1, 0, 5, 17, 16, 0, 6252, 58272, 14400000000ull, 3, 32, 3, 8, 1, 157904, 0, 0, 0, 0, 0, 0, 1, 256, 0, 0}},
    // 32 x 100 kbp semi-global, 288 GB, budget 60 %, a slot per team, level 6
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 0, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 6, 0, 1, 32ull, 100000u},
     {1, 0, 6, 17, 16, 0, 6252, 58272, 21600000000ull, 2, 32, 2, 8, 1, 157904, 0, 0, 0, 0, 0, 0, 1, 256, 0, 0}},
    // 32 x 100 kbp semi-global, 288 GB, budget 60 %, a slot per team, level 7
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 0, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 7, 0, 1, 32ull, 100000u},
     {1, 0, 7, 17, 16, 0, 6252, 58272, 43200000000ull, 1, 32, 1, 8, 1, 157904, 0, 0, 0, 0, 0, 0, 1, 256, 0, 0}},
    // 32 x 100 kbp semi-global, 288 GB, budget 60 %, a slot per team, level 8
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 0, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 8, 0, 1, 32ull, 100000u},
     {0, 0, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}},
    // 32 x 100 kbp semi-global, 288 GB, budget 80 %, a slot per team, level 3
    {{{288000000000ull, 256, 80, 0, 0, 0, 8192, 0, 1, 1, 0, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 3, 0, 1, 32ull, 100000u},
     {1, 0, 3, 17, 16, 0, 6252, 58272, 4915200000ull, 10, 25, 10, 8, 1, 157904, 0, 0, 0, 0, 0, 0, 0, 250, 0, 0}},
    // 32 x 100 kbp semi-global, 288 GB, budget 80 %, a slot per team, level 4
    {{{288000000000ull, 256, 80, 0, 0, 0, 8192, 0, 1, 1, 0, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 4, 0, 1, 32ull, 100000u},
     {1, 0, 4, 17, 16, 0, 6252, 58272, 11520000000ull, 5, 32, 5, 8, 1, 157904, 0, 0, 0, 0, 0, 0, 1, 256, 0, 0}},
    // 32 x 100 kbp semi-global, 288 GB, budget 80 %, a slot per team, level 5
    {{{288000000000ull, 256, 80, 0, 0, 0, 8192, 0, 1, 1, 0, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 5, 0, 1, 32ull, 100000u},
     {1, 0, 5, 17, 16, 0, 6252, 58272, 14400000000ull, 4, 32, 4, 8, 1, 157904, 0, 0, 0, 0, 0, 0, 1, 256, 0, 0}},
    // 32 x 100 kbp semi-global, 288 GB, budget 80 %, a slot per team, level 6
    {{{288000000000ull, 256, 80, 0, 0, 0, 8192, 0, 1, 1, 0, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 6, 0, 1, 32ull, 100000u},
     {1, 0, 6, 17, 16, 0, 6252, 58272, 19200000000ull, 3, 32, 3, 8, 1, 157904, 0, 0, 0, 0, 0, 0, 1, 256, 0, 0}},
    // 32 x 100 kbp semi-global, 288 GB, budget 80 %, a slot per team, level 7
    {{{288000000000ull, 256, 80, 0, 0, 0, 8192, 0, 1, 1, 0, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 7, 0, 1, 32ull, 100000u},
     {1, 0, 7, 17, 16, 0, 6252, 58272, 28800000000ull, 2, 32, 2, 8, 1, 157904, 0, 0, 0, 0, 0, 0, 1, 256, 0, 0}},
    // 32 x 100 kbp semi-global, 288 GB, budget 80 %, a slot per team, level 8
    {{{288000000000ull, 256, 80, 0, 0, 0, 8192, 0, 1, 1, 0, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 8, 0, 1, 32ull, 100000u},
     {1, 0, 8, 17, 16, 0, 6252, 58272, 57600000000ull, 1, 32, 1, 8, 1, 157904, 0, 0, 0, 0, 0, 0, 1, 256, 0, 0}},
    // 32 x 100 kbp semi-global, 288 GB, budget 80 %, a slot per team, level 9
    {{{288000000000ull, 256, 80, 0, 0, 0, 8192, 0, 1, 1, 0, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 9, 0, 1, 32ull, 100000u},
     {0, 0, 9, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}},
    // the same pairs on the paged pool (the default), budget 60 %, level 3
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 3, 0, 1, 32ull, 100000u},
     {1, 0, 3, 17, 16, 0, 6252, 58272, 39277920256ull, 8, 32, 8, 8, 1, 157904, 1, 0, 39277920256ull, 2404352, 26, 585, 1, 256, 0, 0}},
    // the same pairs on the paged pool (the default), budget 60 %, level 4
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 4, 0, 1, 32ull, 100000u},
     {1, 0, 4, 17, 16, 0, 6252, 58272, 43170234368ull, 8, 32, 8, 8, 1, 157904, 1, 0, 43170234368ull, 2404352, 26, 643, 1, 256, 0, 0}},
    // the same pairs on the paged pool (the default), budget 60 %, level 5
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 5, 0, 1, 32ull, 100000u},
     {1, 0, 5, 17, 16, 0, 6252, 58272, 43160616960ull, 4, 32, 4, 8, 1, 157904, 1, 0, 43160616960ull, 2404352, 26, 643, 1, 256, 0, 0}},
    // the same pairs on the paged pool (the default), budget 60 %, level 6
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 6, 0, 1, 32ull, 100000u},
     {1, 0, 6, 17, 16, 0, 6252, 58272, 43155808256ull, 2, 32, 2, 8, 1, 157904, 1, 0, 43155808256ull, 2404352, 26, 643, 1, 256, 0, 0}},
    // the same pairs on the paged pool (the default), budget 60 %, level 7
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 7, 0, 1, 32ull, 100000u},
     {1, 0, 7, 17, 16, 0, 6252, 58272, 43153403904ull, 1, 32, 1, 8, 1, 157904, 1, 0, 43153403904ull, 2404352, 26, 643, 1, 256, 0, 0}},
    // the same pairs on the paged pool (the default), budget 60 %, level 8
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 8, 0, 1, 32ull, 100000u},
     {0, 0, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}},
    // 3 pairs of up to 15 600 bases on a 3 GiB device, start level 2 learned from an earlier call
    {{{3221225472ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 2, 1, 1, 3ull, 15600u},
     {1, 0, 2, 17, 4, 0, 976, 16064, 479281152, 3, 32, 3, 8, 1, 115696, 1, 0, 479281152, 376832, 23, 57, 1, 256, 0, 0}},
    // 3 pairs of up to 15 600 bases on a 3 GiB device, start level 3 learned from an earlier call: no slot fits, the hint climbs down to level 2
    {{{3221225472ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 3, 1, 1, 3ull, 15600u},
     {1, 0, 2, 17, 4, 0, 976, 16064, 479281152, 3, 32, 3, 8, 1, 115696, 1, 0, 479281152, 376832, 23, 57, 1, 256, 0, 0}},
    // 3 pairs of up to 15 600 bases on a 3 GiB device, start level 6 learned from an earlier call: no slot fits, the hint climbs down to level 2
    {{{3221225472ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 6, 1, 1, 3ull, 15600u},
     {1, 0, 2, 17, 4, 0, 976, 16064, 479281152, 3, 32, 3, 8, 1, 115696, 1, 0, 479281152, 376832, 23, 57, 1, 256, 0, 0}},
    // the same at level 6 reached from the failed levels below it (no hint): one team already had the whole pool -- spent, no memory
    {{{3221225472ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 6, 0, 1, 3ull, 15600u},
     {0, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}},
    // ... and without the paged pool: no memory
    {{{3221225472ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 0, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 6, 0, 1, 3ull, 15600u},
     {0, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}},
    // scout pass, 500 x 12 kbp on a 3 GiB device: 48 pages for 256 CUs -- as many scouts as pages
    {{{3221225472ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 1, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 0, 0, 1, 500ull, 12000u},
     {1, 0, 0, 17, 4, 0, 752, 14272, 477102080, 48, 1, 48, 8, 1, 113904, 1, 1, 477102080, 290816, 23, 48, 0, 48, 0, 0}},
    // scout pass, 500 x 12 kbp on 288 GB
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 1, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 0, 0, 1, 500ull, 12000u},
     {1, 0, 0, 0, 4, 0, 751, 14280, 4608000, 500, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 8}},
    // ... the job behind it (pairs the scouts handed on): no scout pass
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 1, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 0, 0, 0, 500ull, 12000u},
     {1, 0, 0, 0, 4, 0, 751, 14280, 4608000, 500, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 8}},
    // team_scout 1 with 12 pairs: not more than two pairs per team, no scout pass
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 1, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 0, 0, 1, 12ull, 12000u},
     {1, 0, 0, 17, 4, 0, 752, 14272, 39026688, 8, 32, 8, 8, 1, 113904, 1, 0, 39026688, 290816, 20, 35, 1, 256, 0, 0}},
    // team_scout 2: whatever the batch size (twelve scouts, and the XCD mapping gives each 32 workgroups' worth of grid)
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 2, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 0, 0, 1, 12ull, 12000u},
     {1, 0, 0, 17, 4, 0, 752, 14272, 58015744, 12, 1, 12, 8, 1, 113904, 1, 1, 58015744, 290816, 20, 52, 0, 12, 0, 0}},
    // 2^27 bases, global: the sequences do not fit LDS -- byte path; wfa_team_kernel (wfa_teamc_kernel stops below 2^27)
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 1, 1}, 0, 0, 0, 1, 2ull, 134217728u},
     {1, 1, 0, 7, 16, 1, 0, 8256, 17179873280ull, 1, 32, 1, 8, 0, 0, 1, 0, 17179873280ull, 3221229568, 30, 13, 1, 256, 0, 0}},
    // 500 x 700 kbp global: byte path
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 1, 1}, 0, 0, 0, 1, 500ull, 700000u},
     {1, 1, 0, 0, 16, 1, 0, 8272, 67200000, 500, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 8}},
    // 12 x 12 kbp semi-global, 288 GB
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 0, 0, 1, 12ull, 12000u},
     {1, 0, 0, 17, 4, 0, 752, 14272, 39026688, 8, 32, 8, 8, 1, 113904, 1, 0, 39026688, 290816, 20, 35, 1, 256, 0, 0}},
    // 12 x 12 kbp global, 288 GB
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 1, 1}, 0, 0, 0, 1, 12ull, 12000u},
     {1, 0, 0, 17, 4, 0, 752, 14272, 10715136, 8, 32, 8, 8, 1, 113904, 1, 0, 10715136, 290816, 20, 8, 1, 256, 0, 0}},
    // 12 x 12 kbp semi-global, 4 GiB
    {{{4294967296ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 0, 0, 1, 12ull, 12000u},
     {1, 0, 0, 17, 4, 0, 752, 14272, 39026688, 8, 32, 8, 8, 1, 113904, 1, 0, 39026688, 290816, 20, 35, 1, 256, 0, 0}},
    // 12 x 12 kbp global, 4 GiB
    {{{4294967296ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 1, 1}, 0, 0, 0, 1, 12ull, 12000u},
     {1, 0, 0, 17, 4, 0, 752, 14272, 10715136, 8, 32, 8, 8, 1, 113904, 1, 0, 10715136, 290816, 20, 8, 1, 256, 0, 0}},
    // 12 x 12 kbp semi-global, 3 GiB
    {{{3221225472ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 0, 0, 1, 12ull, 12000u},
     {1, 0, 0, 17, 4, 0, 752, 14272, 39026688, 8, 32, 8, 8, 1, 113904, 1, 0, 39026688, 290816, 20, 35, 1, 256, 0, 0}},
    // 12 x 12 kbp global, 3 GiB
    {{{3221225472ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 1, 1}, 0, 0, 0, 1, 12ull, 12000u},
     {1, 0, 0, 17, 4, 0, 752, 14272, 10715136, 8, 32, 8, 8, 1, 113904, 1, 0, 10715136, 290816, 20, 8, 1, 256, 0, 0}},
    // 12 x 12 kbp, team_paged 0
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 0, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 0, 0, 1, 12ull, 12000u},
     {1, 0, 0, 17, 4, 0, 752, 14272, 4608000, 12, 6, 12, 8, 1, 113904, 0, 0, 0, 0, 0, 0, 0, 72, 0, 0}},
    // 12 x 12 kbp, team_compact 0: wfa_team_kernel
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 0, 1, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 0, 0, 1, 12ull, 12000u},
     {1, 0, 0, 7, 4, 0, 752, 14272, 39026688, 8, 32, 8, 8, 0, 0, 1, 0, 39026688, 290816, 20, 35, 1, 256, 0, 0}},
    // 12 x 12 kbp, team_wgs 3
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 3, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 0, 0, 1, 12ull, 12000u},
     {1, 0, 0, 17, 4, 0, 752, 14272, 4608000, 12, 3, 12, 8, 1, 113904, 0, 0, 0, 0, 0, 0, 0, 36, 0, 0}},
    // 12 x 12 kbp, arena_bytes_per_slot 16 KiB
    {{{288000000000ull, 256, 60, 16384, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 0, 0, 1, 12ull, 12000u},
     {1, 0, 0, 17, 4, 0, 752, 14272, 4096, 12, 6, 12, 8, 1, 113904, 0, 0, 0, 0, 0, 0, 0, 72, 0, 0}},
    // 12 x 12 kbp on 228 CUs: no XCD mapping
    {{{288000000000ull, 228, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 0, 1}, 0, 0, 0, 1, 12ull, 12000u},
     {1, 0, 0, 17, 4, 0, 752, 14272, 39026688, 8, 6, 8, 8, 1, 113904, 1, 0, 39026688, 290816, 20, 35, 0, 48, 0, 0}},
    // 12 x 12 kbp, gap extension 0: no team kernel, no ring of rows
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 6, 0, 2, 0, 1}, 0, 0, 0, 1, 12ull, 12000u},
     {1, 0, 0, 0, 4, 0, 751, 8136, 4608000, 12, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0}},
    // 12 x 12 kbp, penalties 2/4/1: wfa_teamc_kernel's rings (5 + 2 rows) do not fit, wfa_team_kernel
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 2, 5, 1, 1, 0, 1}, 0, 0, 0, 1, 12ull, 12000u},
     {1, 0, 0, 17, 4, 0, 752, 14272, 39026688, 8, 32, 8, 8, 1, 130296, 1, 0, 39026688, 290816, 20, 35, 1, 256, 0, 0}},
    // 500 x 12 kbp global: one workgroup per pair fills the GPU, wfa_generic_kernel with its wave mode
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 1, 1}, 0, 0, 0, 1, 500ull, 12000u},
     {1, 0, 0, 0, 4, 0, 751, 14280, 1152000, 500, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 8}},
    // 300 x 1 kbp global, team_min_len 0: one wave per pair
    {{{288000000000ull, 256, 60, 0, 0, 0, 0, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 1, 1}, 0, 0, 0, 1, 300ull, 1000u},
     {1, 0, 0, 0, 1, 0, 64, 8784, 96000, 300, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 8}},
    // ... threads_per_pair 256: four
    {{{288000000000ull, 256, 60, 0, 0, 256, 0, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 1, 1}, 0, 0, 0, 1, 300ull, 1000u},
     {1, 0, 0, 0, 4, 0, 64, 8784, 96000, 300, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 8}},
    // 4 096 bases: one wave per pair
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 1, 1}, 0, 0, 0, 1, 20000ull, 4096u},
     {1, 0, 0, 0, 1, 0, 257, 10328, 393216, 8192, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 8}},
    // 4 097 bases: four
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 1, 1}, 0, 0, 0, 1, 20000ull, 4097u},
     {1, 0, 0, 0, 4, 0, 258, 10336, 393312, 2048, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 8}},
    // 65 537 bases: sixteen
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 0, 0, 4, 8, 2, 2, 1, 1}, 0, 0, 0, 1, 20000ull, 65537u},
     {1, 0, 0, 0, 16, 0, 4098, 41056, 6291552, 512, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 8}},
    // the one-pair debug launch: wfa_generic_kernel, one slot
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 0, 1, 1, 1, 0, 2, 1, 0, 4, 8, 2, 2, 0, 1}, 0, 0, 0, 1, 1ull, 12000u},
     {1, 0, 0, 0, 4, 0, 751, 14280, 4608000, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 8}},
    // ... with team_wgs 3: wfa_team_kernel
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 3, 1, 1, 1, 0, 2, 1, 0, 4, 8, 2, 2, 0, 1}, 0, 0, 0, 1, 1ull, 12000u},
     {1, 0, 0, 7, 4, 0, 752, 14272, 4608000, 1, 3, 1, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0, 0}},
    // ... of wfahip_debug_team_compact: wfa_teamc_kernel
    {{{288000000000ull, 256, 60, 0, 0, 0, 8192, 3, 1, 1, 1, 0, 2, 1, 1, 4, 8, 2, 2, 0, 1}, 0, 0, 0, 1, 1ull, 12000u},
     {1, 0, 0, 17, 4, 0, 752, 14272, 4608000, 1, 3, 1, 8, 1, 113904, 0, 0, 0, 0, 0, 0, 0, 3, 0, 0}},
};

// the invariants of a plan that launches; 0 or the one that is broken
const char *broken(const JobIn &j, const LadderPlan &p) {
    const uint64_t cus = (uint64_t)std::max(1, j.env.num_cus), budget = j.env.budget_bytes();
    if ((p.kind == K_TEAMC ? p.lds_c : p.cfg.lds_bytes) > LDS_MAX_BYTES) return "the launch's LDS exceeds LDS_MAX_BYTES";
    if (p.kind != K_GENERIC && j.env.team_wgs == 0 && ((uint64_t)p.grid > cus || (uint64_t)p.team_n * p.team_T > cus)) return "teams x workgroups per team exceed the CUs";
    if (!p.paged && (uint64_t)p.cfg.slots * p.cfg.arena_words * 4ull > budget) return "slots x arena_words x 4 exceeds the budget";
    if (p.paged && p.n_pages < p.team_n) return "fewer pages than teams";
    // (NOT asserted: "a paged pool does not exceed the budget".  Below the first level whose slots no longer fit, the pool is the teams'
    // slots PLUS their directory regions, which the sizing code has always let go over the budget by those regions: 147 456 of the grid's
    // launches, e.g. three 100 kbp global pairs at level 4 on a 3 GiB device -- 1.941 GB against 1.933.)
    return nullptr;
}

}  // namespace

int main() {
    // ---- the literal plans
    int n_rows = 0;
    for (const Row &r : ROWS) {
        uint64_t got[F_COUNT];
        flatten(plan(r.in), got);
        for (int f = 0; f < (r.want[F_LAUNCH] ? (int)F_COUNT : 3); f++)
            if (got[f] != r.want[f]) {
                std::fprintf(stderr, "row %d: %s is %llu, expected %llu\n", n_rows, FIELD[f], (unsigned long long)got[f], (unsigned long long)r.want[f]);
                return 1;
            }
        n_rows++;
    }

    // ---- the figures the comments of ladder_slot_words() and of opt_arena_budget_pct quote: a 100 kbp semi-global pair on a 288 GB device
    {
        LadderEnv E = ROWS[0].in.env;
        const struct { int pct, level; uint64_t slots, gb; } fig[] = {{60, 4, 4, 43}, {60, 5, 3, 57}, {60, 6, 2, 86}, {60, 7, 1, 172},
                                                                      {80, 4, 5, 46}, {80, 5, 4, 57}, {80, 6, 3, 76}, {80, 7, 2, 115}, {80, 8, 1, 230},
                                                                      {85, 4, 6, 40}, {90, 4, 6, 43}};  // ("five or six slots instead of four")
        for (const auto &f : fig) {
            E.arena_budget_pct = f.pct;
            const uint64_t bytes = ladder_slot_words(E, 100000, f.level) * 4ull;
            if (bytes / 1000000000ull != f.gb || E.budget_bytes() / bytes != f.slots) {
                std::fprintf(stderr, "budget %d %%, level %d: a slot of %llu bytes, %llu of them fit; expected %llu x %llu GB\n", f.pct, f.level, (unsigned long long)bytes,
                             (unsigned long long)(E.budget_bytes() / bytes), (unsigned long long)f.slots, (unsigned long long)f.gb);
                return 1;
            }
        }
        for (int pct : {60, 80}) {  // level 3: 19.7 GB, and the level after the last slot has none
            E.arena_budget_pct = pct;
            if (ladder_slot_words(E, 100000, 3) * 4ull != 19660800000ull || ladder_slot_words(E, 100000, pct == 60 ? 8 : 9) * 4ull <= E.budget_bytes()) {
                std::fprintf(stderr, "budget %d %%: level 3 or the level behind the last slot\n", pct);
                return 1;
            }
        }
    }

    // ---- invariants over the grid, and the same plan when asked twice
    const uint64_t mems[] = {3ull << 30, 4ull << 30, 288000000000ull};
    const int      cus_[] = {256, 228};
    const uint32_t lens[] = {1, 4096, 4097, 8191, 8192, 12000, 65536, 65537, 100000, 1u << 27};
    const uint64_t works[] = {1, 2, 3, 12, 32, 500, 20000};
    const uint32_t pens[3][4] = {{4, 8, 2, 2}, {2, 5, 1, 1}, {4, 6, 0, 2}};  // x, o + e, e, g of 4/6/2, 2/4/1 and 4/6/0
    const int64_t  min_lens[] = {0, 1, 8192};
    // team_scout, the job's scout flag, wf-adaptive (which only the scout pass reads: off where that pass would otherwise run)
    const int scouts[8][3] = {{0, 0, 1}, {0, 1, 1}, {1, 0, 1}, {1, 1, 1}, {1, 1, 0}, {2, 0, 1}, {2, 1, 1}, {2, 1, 0}};
    const int dbgs[3][2] = {{0, 0}, {1, 0}, {1, 1}};  // debug_single, dbg_teamc
    std::atomic<int>      next{0};
    std::atomic<uint64_t> n_cases{0}, n_launches{0};
    std::atomic<bool>     failed{false};
    const auto worker = [&]() {
        for (int outer; (outer = next++) < 3 * 10 * 14 && !failed;) {
            JobIn j{};
            j.env.total_mem = mems[outer / 140], j.max_len = lens[outer / 14 % 10], j.level = outer % 14;
            j.env.slots = 0, j.env.threads_per_pair = 0, j.env.team_xcd = 2;
            uint64_t cases = 0, launches = 0, a[F_COUNT], b[F_COUNT];
            for (int cu : cus_) for (int mode = 0; mode < 2; mode++) for (uint64_t nw : works) for (int gl = 0; gl < 2; gl++) for (const auto &pen : pens)
            for (int wgs : {0, 3}) for (int pg = 0; pg < 2; pg++) for (int cp = 0; cp < 2; cp++) for (int wv = 0; wv < 2; wv++) for (const auto &sc : scouts)
            for (int abps : {0, 16384}) for (int pct : {60, 80}) for (int64_t ml : min_lens) for (const auto &dbg : dbgs) for (int hint = 0; hint < 2; hint++) {
                LadderEnv &E = j.env;
                E.num_cus = cu, j.mode = mode, j.n_work = nw, E.global_alignment = gl != 0, E.x = pen[0], E.oe = pen[1], E.e = pen[2], E.g = pen[3];
                E.team_wgs = wgs, E.team_paged = pg, E.team_compact = cp, E.team_wave = wv, E.team_scout = sc[0], j.scout = sc[1], E.adaptive = sc[2] != 0;
                E.arena_bytes_per_slot = abps, E.arena_budget_pct = pct, E.team_min_len = ml, E.debug_single = dbg[0] != 0, E.dbg_teamc = dbg[1] != 0, j.hint = hint;
                const LadderPlan p = plan(j);
                cases++;
                flatten(p, a), flatten(plan(j), b);
                const char *bad = !same(a, b) ? "the plan differs when asked twice" : (p.launch ? broken(j, p) : nullptr);
                launches += p.launch;
                if (bad && !failed.exchange(true))
                    std::fprintf(stderr, "%s: total_mem %llu num_cus %d max_len %u mode %d level %d n_work %llu global %d x %u o+e %u e %u team_wgs %d team_paged %d team_compact %d team_wave %d "
                                 "team_scout %d scout %d adaptive %d arena_bytes_per_slot %d arena_budget_pct %d team_min_len %d debug_single %d dbg_teamc %d hint %d\n", bad,
                                 (unsigned long long)E.total_mem, cu, j.max_len, mode, j.level, (unsigned long long)nw, gl, pen[0], pen[1], pen[2], wgs, pg, cp, wv, sc[0], sc[1], sc[2], abps, pct, (int)ml,
                                 dbg[0], dbg[1], hint);
            }
            n_cases += cases, n_launches += launches;
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < std::min(8u, std::max(1u, std::thread::hardware_concurrency())); t++) pool.emplace_back(worker);
    worker();
    for (std::thread &t : pool) t.join();
    if (failed) return 1;
    if (n_cases != 650280960ull) {
        std::fprintf(stderr, "the grid has %llu cases, expected 650 280 960\n", (unsigned long long)n_cases.load());
        return 1;
    }
    std::printf("ladder host test ok: %d literal plans, %llu grid cases, %llu of them launches\n", n_rows, (unsigned long long)n_cases.load(), (unsigned long long)n_launches.load());
    return 0;
}
