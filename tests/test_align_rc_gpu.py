"""GPU: full alignment of the reverse strand of packed queries (wfahip_align_batch_packed_rc).  Every comparison has three sides: the
new entry on the caller's words with flags; the oracle on bytes reverse-complemented on the host; and the EXISTING packed entry on a
buffer whose flagged queries were reverse-complemented and packed on the host.  Every record field and every CIGAR op must agree,
and so must the route between the first and the third side (main_kernel_kind, n_packed_pairs, n_retried_pairs): the same pairs on
the same kernels, so the cases check for themselves that they reach the pass they name.  The two sides run on aligners of their own
with the same options: what a context learns from a call must not route the second one differently."""
import numpy as np
import pytest

from oracle import oracle as O
from test_parity_gpu import assert_batch_equal
from test_score_rc_gpu import ADAPT, MAX_SEQ_LEN, MODES, _lay, _mutate, _pair_of, _rand, _revcomp, _stored

pytestmark = pytest.mark.gpu
PAIR_EMPTY, PAIR_TOO_LONG = 1, 2


def _aligner(glob, adaptive, opts=None):
    import wfa_amd
    al = wfa_amd.New(wfa_amd.Penalties(4, 6, 2), wfa_amd.Options(GlobalAlignment=glob), device=0)
    if adaptive is not None:
        assert al.AdaptiveReduction(wfa_amd.AdaptiveReductionOption(*adaptive)) is None
    for k, v in (opts or {}).items():
        al.set_option(k, v)
    return al


def _oracle(qs, ts, glob, adaptive):
    import wfa_amd
    return O.align_batch(O.make_params(4, 6, 2, global_alignment=glob, adaptive=adaptive), *wfa_amd.make_blob(qs, ts), n_threads=16)


def _route(t):
    return (t.main_kernel_kind, t.n_packed_pairs, t.n_retried_pairs)


def _three_pk(new_pk, flags, host_pk, want, glob, adaptive, opts=None, what="", als=None, keep=False):
    """the new entry over new_pk with flags; the existing entry over host_pk (flagged queries reverse-complemented on the host); the
    oracle.  Returns the new entry's result, its timing and -- keep, or als given: the aligners of an earlier call -- the two aligners.
    Unless they are kept, the first aligner is closed before the second exists: a context of the long-pair cases holds arenas of
    many GB, and a failing case must not leave them to the tests behind it"""
    al, ref = als or (None, None)
    try:
        al = al or _aligner(glob, adaptive, opts)
        got = al.align_arrays_packed_rc(*new_pk, flags)
        tn = al.last_timing()
        if not (keep or als):
            al.close()
            al = None
        ref = ref or _aligner(glob, adaptive, opts)
        host = ref.align_arrays_packed(*host_pk)
        th = ref.last_timing()
        print(what, "glob", glob, "adaptive", adaptive, "| rc: kind, packed, retried", _route(tn), "| host-materialised:", _route(th))
        assert_batch_equal(got, want, what + ": against the oracle")
        assert_batch_equal(got, host, what + ": against the packed entry on host-made words")
        assert _route(tn) == _route(th), what
    except BaseException:
        keep = als = None
        raise
    finally:
        if not (keep or als):
            for a in (al, ref):
                if a is not None:
                    a.close()
    return got, tn, (al, ref)


def _buffers(logical, ts, flags, gap=0, fill=0):
    """pairs (logical[i], ts[i]): the caller's buffer holds the reverse complement of a flagged pair's query"""
    n = len(ts)
    q_len = np.array([len(q) for q in logical], np.uint32)
    t_len = np.array([len(t) for t in ts], np.uint32)
    packed, offs = _lay(_stored(logical, flags) + list(ts), gap, fill)
    host, hoffs = _lay(list(logical) + list(ts))
    return (packed, offs[:n].copy(), q_len, offs[n:].copy(), t_len), (host, hoffs[:n].copy(), q_len, hoffs[n:].copy(), t_len)


def _three(logical, ts, flags, glob, adaptive, opts=None, what="", gap=0, fill=0, want=None):
    flags = np.asarray(flags, np.uint8)
    new_pk, host_pk = _buffers(logical, ts, flags, gap, fill)
    want = want if want is not None else _oracle(logical, ts, glob, adaptive)
    got, t, _ = _three_pk(new_pk, flags, host_pk, want, glob, adaptive, opts, what)
    return got, t


def _generated(seed, n, length, rate):
    import wfa_amd
    blob, q_off, q_len, t_off, t_len = wfa_amd.generate_pairs(seed=seed, n_pairs=n, length=length, error_rate=rate)
    qs = [bytes(blob[int(o):int(o) + int(k)]) for o, k in zip(q_off, q_len)]
    ts = [bytes(blob[int(o):int(o) + int(k)]) for o, k in zip(t_off, t_len)]
    return qs, ts


def _alternate(n):
    return ((np.arange(n) + 1) % 2).astype(np.uint8)  # the query at word 0 of the buffer is a flagged one


@pytest.mark.parametrize("glob,adaptive", MODES)
def test_word_boundaries(glob, adaptive):
    """every length 1 .. 40, 63 .. 65 and 224 .. 240 (the seam of the packed first pass), zeros and ones in every tail bit, pad word
    and gap word; a flagged query at word 0"""
    rng = np.random.default_rng(51)
    pairs = [_pair_of(rng, ln, 0.06) for ln in list(range(1, 41)) + [63, 64, 65] + list(range(224, 241))]
    qs, ts = [p[0] for p in pairs] * 2, [p[1] for p in pairs] * 2  # every pair under both flags
    flags = _alternate(len(qs))
    want = _oracle(qs, ts, glob, adaptive)
    a, ta = _three(qs, ts, flags, glob, adaptive, what="word boundaries, fill 0", want=want)
    b, tb = _three(qs, ts, flags, glob, adaptive, what="word boundaries, fill 1", gap=1, fill=0xFFFFFFFF, want=want)
    assert_batch_equal(a, b, "tail bits")
    assert _route(ta) == _route(tb)


@pytest.mark.parametrize("glob,adaptive", MODES)
def test_first_pass_slots_1kbp(glob, adaptive):
    """1 000-base pairs at 5 %: wfa_prepack_words_kernel fills the slots of wfa_duo_kernel (global alignment; option duo = 2 gives it the
    pass whatever the batch size) -- the flagged queries' halves reverse-complemented word by word"""
    qs, ts = _generated(52, 520, 1000, 0.05)
    _, t = _three(qs, ts, _alternate(len(qs)), glob, adaptive, {"duo": 2}, "1 kbp at 5 %", fill=0xFFFFFFFF)
    if glob:  # (without wf-adaptive the bands outgrow the kernel's diagonals and it hands the pairs on: the retry rungs, from bytes)
        assert t.main_kernel_kind == 8 and (adaptive is None or (t.n_packed_pairs == len(qs) and t.n_retried_pairs == 0)), t


@pytest.mark.parametrize("glob,adaptive", MODES)
@pytest.mark.parametrize("lane_pack", [1, 0])
def test_lane_kernel_150_bases(glob, adaptive, lane_pack):
    """150-base reads at 2 % on wfa_lane_kernel (option lane = 2): packing the bytes itself -- its pairs are expanded first, the flagged
    queries into the mirror -- and from the slots of wfa_prepack_words_kernel (lane_pack = 0)"""
    qs, ts = _generated(53, 1500, 150, 0.02)
    _, t = _three(qs, ts, _alternate(len(qs)), glob, adaptive, {"lane": 2, "lane_pack": lane_pack}, f"150 bases, lane_pack {lane_pack}", fill=0xFFFFFFFF)
    if glob:
        assert t.main_kernel_kind == 10, t


@pytest.mark.parametrize("glob,adaptive", MODES)
@pytest.mark.parametrize("bins", [False, True])
def test_wide_kernel_and_its_hand_on(glob, adaptive, bins):
    """2 040 .. 2 060 bases among 300-base reads: semi-global, wfa_wide_kernel's packed prologue takes the reads up to 2 047 bases and the
    ladder the longer ones; with wide_bin_min_pairs lowered the batch is cut into length classes first"""
    rng = np.random.default_rng(54)
    pairs = [_pair_of(rng, ln, 0.03) for ln in range(2040, 2061)] + [_pair_of(rng, int(rng.integers(200, 400)), 0.04) for _ in range(90)]
    order = rng.permutation(len(pairs))
    qs, ts = [pairs[i][0] for i in order], [pairs[i][1] for i in order]
    opts = {"wide_bin_min_pairs": 1} if bins else {}
    _, t = _three(qs, ts, _alternate(len(qs)), glob, adaptive, opts, f"2040..2060, classes {bins}", fill=0xFFFFFFFF)
    if not glob:
        assert t.main_kernel_kind == 18 and t.n_retried_pairs >= 13, t


@pytest.mark.parametrize("glob,adaptive", MODES)
def test_long_windows_and_their_rungs(glob, adaptive):
    """eight 12 000-base pairs mixed into 300 of 1 000 bases (tests/test_rungs_gpu.py): the short pairs' pass hands the long ones on,
    they take the sliding-window passes from slots and what leaves those the next rung and the ladder, from bytes"""
    short = _generated(55, 300, 1000, 0.05)
    longp = _generated(56, 8, 12000, 0.05)
    qs, ts = short[0] + longp[0], short[1] + longp[1]
    flags = _alternate(len(qs))
    flags[300:] = [1, 0, 1, 1, 0, 1, 0, 1]
    # (team_paged 0: the teams of the ladder own a slot each.  With the paged pool, how many of the 12 000-base pairs run out of pages and
    # are counted once more depends on which teams hold pages at that moment -- without wf-adaptive the packed entry itself reports 313 or
    # 314 retried pairs from run to run on this batch, and 316 every time with slots)
    opts = {"team_paged": 0, "duo": 0} if glob else {"team_paged": 0}
    _, t = _three(qs, ts, flags, glob, adaptive, opts, "long pairs among short ones", fill=0xFFFFFFFF)
    if glob:
        assert t.n_retried_pairs >= 8, t


@pytest.mark.parametrize("glob,adaptive", MODES)
def test_team_kernels(glob, adaptive):
    """700-base pairs at 10 % forced onto the team kernels (packed 0, team_min_len 1, as test_parity_gpu.test_team_kernel_small):
    the ladder expands its job's pairs"""
    qs, ts = _generated(57, 6, 700, 0.10)
    opts = {"packed": 0, "team_min_len": 1, "team_wgs": 3, "team_solo_max": 16}
    _three(qs, ts, [1, 0, 1, 1, 0, 1], glob, adaptive, opts, "team kernels", fill=0xFFFFFFFF)


@pytest.mark.parametrize("glob", [True, False])
def test_retry_rungs_at_10_percent(glob):
    """10 % error with wf-adaptive off: the bands outgrow the first pass and the pairs climb the retry rungs, which read bytes"""
    qs, ts = _generated(58, 400, 1000, 0.10)
    _, t = _three(qs, ts, _alternate(len(qs)), glob, None, {}, "10 % without wf-adaptive", fill=0xFFFFFFFF)
    if glob:
        assert t.n_retried_pairs > 0, t


@pytest.mark.parametrize("glob,adaptive", MODES)
@pytest.mark.parametrize("slots", [False, True])
def test_one_query_listed_six_times(glob, adaptive, slots):
    """one stored query: forward, flagged, flagged at a shorter length, forward at that length, flagged from a word offset inside it, and
    a flagged palindrome -- in a batch whose pass reads bytes and in one whose pass copies slots (duo = 2).  The flagged listings share
    mirror bytes under three different lengths"""
    rng = np.random.default_rng(59)
    L, S, W = 1000, 613, 7  # full length, the shorter one, the word offset inside the query
    stored = _rand(rng, L)
    pal = b"ACGT" * 100
    assert _revcomp(pal) == pal
    logical = [stored, _revcomp(stored), _revcomp(stored[:S]), stored[:S], _revcomp(stored[16 * W:]), pal]
    listing = [(0, L, 0), (0, L, 1), (0, S, 1), (0, S, 0), (W, L - 16 * W, 1), (None, len(pal), 1)]
    filler = _generated(60, 260, 1000, 0.05)
    ts = [_mutate(rng, q, 0.05) for q in logical]
    seqs = [stored, pal] + ts + filler[0] + filler[1]  # every sequence ONCE
    packed, offs = _lay(seqs, gap=1, fill=0xFFFFFFFF)
    n6, nf = len(logical), len(filler[0])
    q_woff = np.array([int(offs[1]) if w is None else int(offs[0]) + w for w, _, _ in listing] + [int(o) for o in offs[2 + n6:2 + n6 + nf]], np.uint64)
    t_woff = np.array([int(o) for o in offs[2:2 + n6]] + [int(o) for o in offs[2 + n6 + nf:]], np.uint64)
    q_len = np.array([ln for _, ln, _ in listing] + [len(q) for q in filler[0]], np.uint32)
    t_len = np.array([len(t) for t in ts + filler[1]], np.uint32)
    flags = np.array([f for _, _, f in listing] + [0] * nf, np.uint8)
    all_q, all_t = logical + filler[0], ts + filler[1]
    host_pk = _buffers(all_q, all_t, np.zeros(len(all_q), np.uint8))[1]
    opts = {"duo": 2} if slots else {"duo": 0, "prepack": 0}
    got, t, als = _three_pk((packed, q_woff, q_len, t_woff, t_len), flags, host_pk, _oracle(all_q, all_t, glob, adaptive), glob, adaptive, opts,
                            f"six listings, slots {slots}", keep=True)
    if glob and slots:
        assert t.main_kernel_kind == 8, t
    # a flagged palindrome aligns like itself forward
    flags2 = flags.copy()
    flags2[5] = 0
    again = als[0].align_arrays_packed_rc(packed, q_woff, q_len, t_woff, t_len, flags2)
    assert_batch_equal(again, got, "palindrome, unflagged")
    for a in als:
        a.close()


@pytest.mark.parametrize("glob,adaptive", MODES)
def test_empty_and_too_long_pairs(glob, adaptive):
    """set flags on empty and too long pairs, their offsets far outside the buffer: never looked at"""
    rng = np.random.default_rng(61)
    qs = [_rand(rng, int(rng.integers(100, 400))) for _ in range(24)]
    ts = [_mutate(rng, q, 0.05) for q in qs]
    qs[2], ts[5] = b"", b""
    flags = (np.arange(24) % 2).astype(np.uint8)
    flags[[2, 5, 6]] = 1
    new_pk, host_pk = _buffers(qs, ts, flags, fill=0xFFFFFFFF)
    for pk in (new_pk, host_pk):
        pk[2][6] = MAX_SEQ_LEN + 1  # too long
        pk[1][6], pk[1][2] = np.uint64(1 << 40), np.uint64((1 << 64) - 1)
        pk[3][2], pk[3][5] = np.uint64(1 << 41), np.uint64(1 << 63)
    # the oracle's answer, the pair made too long put right: an empty record
    qs_o, ts_o = list(qs), list(ts)
    qs_o[6] = b""
    want = _oracle(qs_o, ts_o, glob, adaptive)
    want.status[6] = PAIR_TOO_LONG
    got, _, _ = _three_pk(new_pk, flags, host_pk, want, glob, adaptive, None, "empty and too long")
    assert got.status[2] == PAIR_EMPTY and got.status[5] == PAIR_EMPTY and got.status[6] == PAIR_TOO_LONG


@pytest.mark.parametrize("glob,adaptive", MODES)
def test_stale_mirror(glob, adaptive):
    """a second, smaller call with other data on the same aligners: nothing of the first call's mirror may be read"""
    qs, ts = _generated(62, 300, 400, 0.10)
    flags = _alternate(len(qs))
    new_pk, host_pk = _buffers(qs, ts, flags, fill=0xFFFFFFFF)
    _, _, als = _three_pk(new_pk, flags, host_pk, _oracle(qs, ts, glob, adaptive), glob, adaptive, {"learn": 0}, "first call", keep=True)
    qs2, ts2 = _generated(63, 120, 390, 0.10)
    flags2 = (np.arange(len(qs2)) % 3 != 0).astype(np.uint8)
    new2, host2 = _buffers(qs2, ts2, flags2)
    _three_pk(new2, flags2, host2, _oracle(qs2, ts2, glob, adaptive), glob, adaptive, None, "second call", als=als)
    for a in als:
        a.close()


@pytest.mark.parametrize("glob,adaptive", MODES)
def test_unpack_all(glob, adaptive):
    """option unpack_all = 1: the whole blob and, with flags, the whole mirror are expanded up front; every pass reads bytes"""
    rng = np.random.default_rng(64)
    pairs = [_pair_of(rng, int(rng.integers(1, 700)), 0.05) for _ in range(200)] + [_pair_of(rng, 2050, 0.03)]
    qs, ts = [p[0] for p in pairs], [p[1] for p in pairs]
    _three(qs, ts, _alternate(len(qs)), glob, adaptive, {"unpack_all": 1}, "unpack_all", gap=1, fill=0xFFFFFFFF)


@pytest.mark.parametrize("glob,adaptive", MODES)
def test_no_flags_is_the_packed_entry(glob, adaptive):
    """q_rc=None and all-zero flags against align_arrays_packed: the same records, ops and timing fields"""
    qs, ts = _generated(65, 300, 500, 0.05)
    pk = _buffers(qs, ts, np.zeros(len(qs), np.uint8))[1]
    want = _oracle(qs, ts, glob, adaptive)
    fields = ("n_launches", "n_retried_pairs", "arena_bytes", "n_main_launches", "n_packed_pairs", "main_kernel_kind", "ops_written", "cells_stored",
              "ladder_start_level")
    seen = []
    for how in ("packed", "none", "zeros"):
        al = _aligner(glob, adaptive)
        got = (al.align_arrays_packed(*pk) if how == "packed" else
               al.align_arrays_packed_rc(*pk, None if how == "none" else np.zeros(len(qs), np.uint8)))
        assert_batch_equal(got, want, how)
        t = al.last_timing()
        seen.append(tuple(getattr(t, f) for f in fields))
        al.close()
    assert seen[0] == seen[1] == seen[2], seen
