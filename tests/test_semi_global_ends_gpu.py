"""GPU: where a semi-global backtrace starts (backtraceStartPosistion, wfa.go:270-375), on the long-pair kernels.  The device has
five restatements of that function that share no code -- the serial one (wfa_device.hpp), the all-threads one of
wfa_generic_kernel, the whole-team one of wfa_team_kernel, and the two found in flight, wfa_wide_kernel's and wfa_teamc_kernel's
(per-score atomic minima fed from every stepping mode and every workgroup's stripe, read back when the pair is over) -- and the
rest of the suite runs the team kernels on wfa_amd.generate_pairs alone, whose alignments end on the final diagonal at the final
score.  The batches of tests/semi_global_ends.py end elsewhere (tests/test_semi_global_ends.py counts, from the oracle, how many
pairs do what), and every route below has to return the oracle's records on them: every field and every CIGAR op, twice through
one aligner over a poisoned arena, with the kernel of the batch pinned (main_kernel_kind: 0 wfa_generic_kernel, 7
wfa_team_kernel, 17 wfa_teamc_kernel).  All routes set packed = 0, which also keeps the batch off wfa_wide_kernel; what a route
hands up the arena ladder (n_retried_pairs) and its launches are printed, not asserted."""
import ctypes as C
import functools

import numpy as np
import pytest

from semi_global_ends import TC_STRIPE, ends_adapt, ends_free
from test_parity_gpu import FIELDS, _aligner, _oracle_params, assert_batch_equal

pytestmark = pytest.mark.gpu
ADAPT = (10, 50, 1)
BATCHES = {"free": (ends_free, None), "adapt": (ends_adapt, ADAPT)}
NAMES = ["free", "adapt"]


@functools.lru_cache(maxsize=None)
def _want(name, pen=(4, 6, 2)):
    """the oracle's records of a batch under one penalty set: computed once, shared by every case that runs it"""
    from oracle import oracle as O
    build, ad = BATCHES[name]
    want = O.align_batch(_oracle_params(False, ad, pen), *build()[0], n_threads=8)
    assert not np.any(want.status)
    return want


def _run(name, pen, opts, kind, what):
    """the batch twice through one aligner with `opts` over a poisoned arena: kind, records, CIGARs; the last run's records"""
    build, ad = BATCHES[name]
    data, want = build()[0], _want(name, pen)
    al = _aligner(False, ad, pen)
    for k, v in {"packed": 0, "arena_poison": 1, **opts}.items():
        al.set_option(k, v)
    try:
        for rep in range(2):
            got = al.align_arrays(*data)
            tm = al.last_timing()
            print(f"{what} batch={name} pen={pen} rep={rep}: kind {tm.main_kernel_kind}, handed on {tm.n_retried_pairs}, launches {tm.n_launches}")
            assert tm.main_kernel_kind == kind, (what, tm.main_kernel_kind)
            assert_batch_equal(got, want, f"{what} batch={name} pen={pen} rep={rep}")
    finally:
        al.close()
    return got


# ---- 1. wfa_generic_kernel: one workgroup of 1, 4 or 16 waves per pair; its wave mode on and off
GENERIC = [(tpp, wave, (4, 6, 2)) for tpp in (64, 256, 1024) for wave in (1, 0)] + [(256, 1, (2, 4, 2))]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("tpp,wave,pen", GENERIC)
def test_generic_kernel(built, tpp, wave, pen, name):
    _run(name, pen, {"team_min_len": 0, "threads_per_pair": tpp, "team_wave": wave}, 0, f"generic tpp={tpp} wave={wave}")


# ---- 2. wfa_team_kernel: team mode for every row (solo_max 0), switches between team and solo mode (16), solo mode (4096)
TEAM = [(wgs, solo, wave, (4, 6, 2)) for wgs, solo in ((2, 0), (5, 16), (3, 4096)) for wave in (1, 0)] + [(3, 4096, 1, (6, 4, 2))]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("wgs,solo_max,wave,pen", TEAM)
def test_team_kernel(built, wgs, solo_max, wave, pen, name):
    _run(name, pen, {"team_min_len": 1, "team_compact": 0, "team_wgs": wgs, "team_solo_max": solo_max, "team_wave": wave}, 7,
         f"team T={wgs} solo_max={solo_max} wave={wave}")


# ---- 3. wfa_teamc_kernel: (team_wgs, team_fast, team_pipe, team_solo_max or None for its default, team_slack, penalties).  The three
# step variants are those of test_teamc_kernel_words_and_results: pipelined steps, general steps only, short steps without the pipeline
STEPS = ((1, 1), (0, 1), (1, 0))
TEAMC = ([(wgs, fast, pipe, None, 1024, (4, 6, 2)) for wgs in (2, 3, 5) for fast, pipe in STEPS] +
         [(3, 1, 1, solo, 1024, (4, 6, 2)) for solo in (0, 64, 4096)] + [(3, 1, 1, None, 3, (4, 6, 2))] +
         [(3, 1, 1, None, 1024, pen) for pen in ((2, 4, 2), (6, 4, 2))])


def _teamc_opts(wgs, fast, pipe, solo_max, slack):
    opts = {"team_min_len": 1, "team_compact": 1, "team_wgs": wgs, "team_fast": fast, "team_pipe": pipe, "team_slack": slack}
    if solo_max is not None:
        opts["team_solo_max"] = solo_max
    return opts


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("wgs,fast,pipe,solo_max,slack,pen", TEAMC)
def test_teamc_kernel(built, wgs, fast, pipe, solo_max, slack, pen, name):
    _run(name, pen, _teamc_opts(wgs, fast, pipe, solo_max, slack), 17, f"teamc T={wgs} fast={fast} pipe={pipe} solo_max={solo_max} slack={slack}")


# ---- 4. the paged pool and the scout pass: the team's size left to the plan
@pytest.mark.parametrize("name,opts", [("adapt", {}), ("free", {}), ("adapt", {"team_scout": 2}), ("free", {"team_paged": 0})])
def test_teamc_kernel_paged_pool_and_scout(built, name, opts):
    _run(name, (4, 6, 2), {"team_min_len": 1, "team_wgs": 0, **opts}, 17, f"teamc, team size by the plan, {opts}")


# ---- 5. one pair at a time through the debug entry of wfa_teamc_kernel
def _seqs(data, i):
    blob, q_off, q_len, t_off, t_len = data
    return (blob[int(q_off[i]):int(q_off[i]) + int(q_len[i])].tobytes(), blob[int(t_off[i]):int(t_off[i]) + int(t_len[i])].tobytes())


def _debug_pair(al, q, t):
    """wfahip_debug_team_compact for its result alone: Aligner.debug_team_compact also turns every arena word of the pair into
    a Python dict entry -- 1e7 of them for the pairs whose hit lies a stripe from Ak.  (The kernel's debug words -- final
    score, start score, start diagonal -- do not come back through this entry; the record's score and tend - qend stand in.)"""
    from wfa_amd import _lib as L
    from wfa_amd.aligner import BatchResult
    rows, words = C.POINTER(L.Row)(), C.POINTER(C.c_uint32)()
    n_rows, n_words = C.c_uint64(), C.c_uint64()
    res = L.Results()
    prm = al._params()
    L.check(L.lib().wfahip_debug_team_compact(al._ctx, C.byref(prm), q, len(q), t, len(t), C.byref(rows), C.byref(n_rows),
                                              C.byref(words), C.byref(n_words), C.byref(res)), "wfahip_debug_team_compact")
    try:
        assert n_rows.value > 0 and n_words.value > 0
        return BatchResult.from_c(res, 1).result(0)
    finally:
        L.lib().wfahip_free(rows)
        L.lib().wfahip_free(words)
        L.lib().wfahip_results_free(C.byref(res))


def test_teamc_kernel_one_pair_at_a_time(built):
    """two pairs of ends_free() from each class of the CPU test -- K < Ak, K > Ak, K == Ak, |K - Ak| >= 4 096, Ak on a stripe's
    edge, rows of three stripes -- and two repeats that start on Ak + 1 (both scans end in a hit at the same score, the upward
    one wins), alone on a team of three: score, CIGAR, match region and statistics"""
    data, kinds = ends_free()
    want = _want("free")
    n, m = data[2].astype(int), data[4].astype(int)
    Ak, K = m - n, want.tend.astype(int) - want.qend.astype(int)
    classes = {"K < Ak": (K < Ak) & (np.abs(K - Ak) < TC_STRIPE), "K > Ak": (K > Ak) & (np.abs(K - Ak) < TC_STRIPE), "K == Ak": (K == Ak) & (n != m),
               "far": np.abs(K - Ak) >= TC_STRIPE, "edge": np.array([k.startswith("edge") for k in kinds]), "three stripes": n + m - 1 > 2 * TC_STRIPE,
               "upward scan wins": (K == Ak + 1) & np.array([k.startswith("repeat") for k in kinds])}
    picked = []
    for what, mask in classes.items():
        idx = [int(i) for i in np.nonzero(mask)[0] if int(i) not in picked]
        assert len(idx) >= 2, what
        picked += [idx[0], idx[-1]]
    al = _aligner(False, None)
    for k, v in {"packed": 0, "arena_poison": 1, **_teamc_opts(3, 1, 1, None, 1024)}.items():
        al.set_option(k, v)
    try:
        for i in picked:
            r = _debug_pair(al, *_seqs(data, i))
            print(f"pair {i} ({kinds[i]}): n {n[i]} m {m[i]} Ak {Ak[i]}, start diagonal {r.TEnd - r.QEnd} (oracle {K[i]}), score {r.Score} (oracle {want.score[i]})")
            assert (r.Score, r.TEnd - r.QEnd) == (int(want.score[i]), int(K[i])), (i, kinds[i])
            assert r.CIGAR(False) == want.cigar(i), (i, kinds[i])
            assert (r.QBegin, r.QEnd, r.TBegin, r.TEnd, r.AlignLen, r.Matches, r.Gaps, r.GapRegions) == tuple(
                int(getattr(want, f)[i]) for f in ("qbegin", "qend", "tbegin", "tend", "align_len", "matches", "gaps", "gap_regions")), (i, kinds[i])
    finally:
        al.close()


# ---- 6. the routes against each other
def _differ(a, b):
    """the pairs at which two sets of records differ in a field or a CIGAR op"""
    bad = np.zeros(len(a.status), dtype=bool)
    for f in ("status",) + FIELDS:
        bad |= getattr(a, f) != getattr(b, f)
    for i in np.nonzero(~bad)[0]:
        bad[i] = not np.array_equal(a.pair_ops(int(i)), b.pair_ops(int(i)))
    return [int(i) for i in np.nonzero(bad)[0]]


@pytest.mark.parametrize("name", NAMES)
def test_routes_agree(built, name):
    """wfa_generic_kernel, wfa_team_kernel and wfa_teamc_kernel on one setting per batch: which route stands alone is said before
    any of them is held against the oracle"""
    build, ad = BATCHES[name]
    data, kinds = build()
    routes = {"generic": ({"team_min_len": 0, "threads_per_pair": 256}, 0),
              "team": ({"team_min_len": 1, "team_compact": 0, "team_wgs": 3, "team_solo_max": 64}, 7),
              "teamc": (_teamc_opts(3, 1, 1, 64, 1024), 17)}
    got = {}
    for route, (opts, kind) in routes.items():
        al = _aligner(False, ad)
        for k, v in {"packed": 0, "arena_poison": 1, **opts}.items():
            al.set_option(k, v)
        got[route] = al.align_arrays(*data)
        tm = al.last_timing()
        print(f"{route} batch={name}: kind {tm.main_kernel_kind}, handed on {tm.n_retried_pairs}, launches {tm.n_launches}")
        assert tm.main_kernel_kind == kind, route
        al.close()
    got["oracle"] = _want(name)
    diff = {(a, b): _differ(got[a], got[b]) for a in got for b in got if a < b}
    diff = {ab: [(i, kinds[i]) for i in bad[:6]] for ab, bad in diff.items() if bad}
    assert not diff, f"batch {name}: records differ between {diff}"
