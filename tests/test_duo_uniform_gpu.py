"""GPU: the wave-uniform tests and the lane constants of wfa_duo_kernel's score step (wfa_duo.hpp; WFA_DUO_UNIFORM in wfa_duo_cfg.hpp).
"Does any running lane ...?" is asked of lane masks by the scalar unit, the masks of the running and of the wide lanes live in scalar
registers, and the lane's diagonal indices, its diagonals and the upper edge of its window are formed by set_derived() and by nothing
else.  Nothing but speed may depend on it; what can go wrong is a test that reads the wrong lanes, and a mask or a constant that is
stale after a pair has widened, narrowed, recentred, parked, resumed, finished or started.

Every test: option duo = 2 (the variable-lanes kernel forced on small batches), records and CIGAR ops of EVERY pair against the oracle,
wfahip_last_timing names the variable-lanes kernel (kind 8) as the main kind, and no more pairs are handed on to the retry rung than the
library handed on before the change -- a wrong result cannot hide there.  Every batch but one has at most eight pairs per wave of the
launch, which makes the pairs of a wave, and with them the hand-ons, the same in every run (a wave starts with queue entries
[8 w, 8 w + 8), wfa_duo.hpp).  Counts of the library before the change, measured on an MI355X (HANDED_ON below; the library after it
gave the same count in every case): 0 in every case of test_seed and test_finish_together_and_in_turn, of test_sequence_ends at
|m - n| = 0, 1 and 7, of test_band_moves at 5 % error and at 8 % under 2/4/2 and 1/1/1, and of test_ragged_lengths with 8 G + 64 pairs
(three runs each) and with 520 under 2/4/2.  Not 0: test_band_moves at 8 % error under 4/6/2 -- 2 of 64, 10 of 200, 19 of 520, the fewest of
six generator seeds each, 5 % of the pairs hand on at that error rate -- test_ragged_lengths 1 of 520 under 4/6/2, test_sequence_ends at
|m - n| = 40 all 24 (a gap of 40 diagonals does not fit a row: these pairs check the step up to the hand-on, and the retry rung's
result), test_out_of_arena_rows 260 of 520 (every 5 % pair, no other).

Cases, at the smallest shapes at which each changed site can go wrong:
  * the seed test (one compare on the step's path, the exact test behind it): pairs whose first bases match and pairs whose first
    bases differ, on the six penalty shapes -- the mismatch seed belongs to step x / g, which differs per shape -- at 260 and 1 000
    bases, 1 .. 17 pairs: a wave that holds a single pair has `run` false in 56 of its lanes, one that holds eight in none;
  * the ends of the sequences (hit_any, slow_any, the termination test and the finish): pairs whose text is 0, 1, 7 and 40 bases
    longer or shorter than the pattern, so that the shorter sequence ends first and the last diagonal is off the main one, with
    wf-adaptive on and off;
  * finishes: eight copies of one pair at six pairs per fetch -- the pairs of a fetch start in the same round and finish in the same
    step, both halves of a row among them -- and at one pair per fetch, where they start and finish on consecutive steps;
  * the hoisted constants: 1 kbp pairs at 5 % and 8 % error, 64 .. 520 of them on one wave per CU, which widen, narrow, recentre, park
    and resume, on ring depths 2, 3 and 4; and ragged lengths of 240 .. 1 950 bases in one batch, where a freed half row resumes or
    starts a pair of another length -- once with eight pairs per wave at most, once with 8 G + 64 pairs on G waves, so that the last
    pairs are claimed from the queue and staged behind running ones;
  * no_room: 96 arena rows a pair -- the 5 % pairs run out of rows and are handed on (ST_REDO_ARENA), the 2 % pairs between them fit.
"""
import functools

import numpy as np
import pytest

from test_duo_claim_gpu import FIELDS, PINNED, _flat_ops, _grid

pytestmark = pytest.mark.gpu

AD = (10, 50, 1)
SHAPES = {"2:4": (4, 6, 2), "1:3": (2, 4, 2), "1:2": (1, 1, 1), "2:3": (4, 4, 2), "2:2": (4, 2, 2), "3:3": (6, 4, 2)}
SHORT = (("duo_short", 2),)
ORACLE_THREADS = 4
KIND_DUO = 8
SEED_SIZES = (1, 2, 3, 8, 9, 17)
ENDS, ENDS_PEN = (0, 1, 7, 40), ((4, 6, 2), (2, 4, 2))
COPIES = (("copies-264", 8), ("copies-264", 17), ("copies-1k", 8), ("copies-1k", 16))
BAND_SHAPES, BAND_SIZES = ("2:4", "1:3", "1:2"), (64, 200, 520)
# which of the generator's seeds test_band_moves uses (the one of six on which the library before the change handed on the fewest pairs)
BAND_SEED = {("1k5", 64): 2, ("1k5", 200): 1, ("1k5", 520): 1, ("1k8", 64): 2, ("1k8", 200): 1, ("1k8", 520): 5}
# Pairs the library handed on to the retry rung BEFORE the change, measured on an MI355X: (kind, n, length, penalties, wf-adaptive on) -> count;
# a case that is not listed handed on none.  Every listed batch has at most eight pairs per wave, so the count is the same in every run.
HANDED_ON = {
    # 8 % error under 4/6/2: bands that outgrow a row, widening pairs that find the wave's park records full (none under 2/4/2 and 1/1/1)
    ("1k8", 64, 2, (4, 6, 2), True): 2, ("1k8", 200, 1, (4, 6, 2), True): 10, ("1k8", 520, 5, (4, 6, 2), True): 19,
    ("ragged", 520, 5, (4, 6, 2), True): 1,
    # a difference of 40 bases takes the band of every pair past the 56 diagonals a row holds: all handed on, with and without wf-adaptive
    ("ends", 24, 40, (4, 6, 2), True): 24, ("ends", 24, 40, (2, 4, 2), True): 24,
    ("ends", 24, 40, (4, 6, 2), False): 24, ("ends", 24, 40, (2, 4, 2), False): 24,
    ("rows", 520, 0, (4, 6, 2), True): 260,  # every 5 % pair, no other
}


def _frozen(data):
    for a in data:
        a.setflags(write=False)
    return tuple(data)


def _blob_of(qs, ts):
    import wfa_amd as w
    return _frozen(w.make_blob(qs, ts))


def _mutate(rng, q, err):
    t = list(q)
    for _ in range(int(round(len(q) * err))):
        kind, pos = int(rng.integers(0, 3)), int(rng.integers(1, max(2, len(t) - 1)))
        if kind == 0:
            t[pos] = (t[pos] + 1 + int(rng.integers(0, 3))) & 3
        elif kind == 1:
            t.insert(pos, int(rng.integers(0, 4)))
        elif len(t) > 2:
            del t[pos]
    return t


_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _bytes(codes):
    return _ACGT[np.asarray(codes, dtype=np.int64) & 3].tobytes()


@functools.lru_cache(maxsize=None)
def _batch(kind, n, length=0):
    """the batches of this file (built once, read only)"""
    import wfa_amd as w
    if kind == "first-base":  # n pairs of `length` bases at 4 % error; the odd ones' texts start with another base than their patterns
        rng = np.random.default_rng(7100 + length + n)
        qs, ts = [], []
        for i in range(n):
            q = list(rng.integers(0, 4, length))
            t = _mutate(rng, q, 0.04)
            t[0] = q[0] if i % 2 == 0 else (q[0] + 1 + i // 2 % 3) & 3
            qs.append(_bytes(q)), ts.append(_bytes(t))
        return _blob_of(qs, ts)
    if kind == "ends":  # pairs of about 300 and about 1 000 bases in turn, the text `length` bases longer (even pairs) or shorter than the pattern
        # (three or four edits a pair, so that without wf-adaptive too the band stays inside a row's 64 diagonals)
        d = length
        rng = np.random.default_rng(7300 + d)
        qs, ts = [], []
        for i in range(n):
            L = (300, 1000)[i // 2 % 2] + int(rng.integers(0, 24))
            q = list(rng.integers(0, 4, L))
            t = _mutate(rng, q, 0.01 if L < 500 else 0.004)
            want_len = L + d if i % 2 == 0 else L - d
            at_start = d <= 7 and i % 3 == 0  # (the difference at the end of the text, or -- the small ones -- at its start for every third pair)
            while len(t) > want_len:
                del t[0 if at_start else -1]
            while len(t) < want_len:
                t.insert(0 if at_start else len(t), int(rng.integers(0, 4)))
            qs.append(_bytes(q)), ts.append(_bytes(t))
        return _blob_of(qs, ts)
    if kind in ("copies-264", "copies-1k"):  # n copies of one pair: 264 bases (six pairs per fetch) or 1 kbp (one pair per fetch), three or four edits
        L = 264 if kind == "copies-264" else 1000
        blob, q_off, q_len, t_off, t_len = w.generate_pairs(seed=7500 + L, n_pairs=1, length=L, error_rate=0.012 if L < 500 else 0.004, n_threads=1)
        one = lambda a: np.full(n, a[0], dtype=a.dtype)
        return _frozen((blob, one(q_off), one(q_len), one(t_off), one(t_len)))
    if kind in ("1k5", "1k8"):  # 1 kbp at 5 % / 8 % error (`length`: which seed)
        return _frozen(w.generate_pairs(seed=7700 + 10 * n + length, n_pairs=n, length=1000, error_rate=0.08 if kind == "1k8" else 0.05, n_threads=4))
    if kind == "ragged":  # 240 .. 1 950 bases at `length` per cent error, the lengths in no order
        rng = np.random.default_rng(7900 + n)
        qs, ts = [], []
        for i in range(n):
            L = int(rng.integers(240, 1951)) if i % 5 else (240, 1950, 1000, 1949, 241)[i // 5 % 5]
            q = list(rng.integers(0, 4, L))
            t = _mutate(rng, q, length / 100.0)[:1950]
            qs.append(_bytes(q)), ts.append(_bytes(t))
        return _blob_of(qs, ts)
    if kind == "rows":  # 2 % and 5 % error in turn: under 4/6/2 at most 20 * 8 / 2 = 80 score steps, and about 160
        parts = [w.generate_pairs(seed=8100 + k, n_pairs=(n - k + 1) // 2, length=1000, error_rate=e, n_threads=4) for k, e in enumerate((0.02, 0.05))]
        base = np.array([0, len(parts[0][0])], dtype=np.uint64)
        blob = np.concatenate([parts[0][0], parts[1][0], np.zeros(16, dtype=np.uint8)])
        q_off, t_off = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        q_len, t_len = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        for k, p in enumerate(parts):
            q_off[k::2], q_len[k::2], t_off[k::2], t_len[k::2] = p[1] + base[k], p[2], p[3] + base[k], p[4]
        return _frozen((blob, q_off, q_len, t_off, t_len))
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _want(kind, n, length, pen, ad):
    """the oracle's records and ops of a batch (computed once, read only)"""
    from oracle import oracle as O
    want = O.align_batch(O.make_params(*pen, global_alignment=True, adaptive=ad), *_batch(kind, n, length), n_threads=ORACLE_THREADS)
    return want, _flat_ops(want)


def _run(kind, n, length, pen, ad, opts):
    """the batch through wfa_duo_kernel: (result, timing)"""
    import wfa_amd as w
    al = w.New(w.Penalties(*pen), w.Options(GlobalAlignment=True), device=0)
    if ad is not None:
        assert al.AdaptiveReduction(w.AdaptiveReductionOption(*ad)) is None
    al.set_option("duo", 2)
    al.set_option("arena_poison", 1)
    for k, v in opts:
        al.set_option(k, v)
    got = al.align_arrays(*_batch(kind, n, length))
    tm = al.last_timing()
    al.close()
    return got, tm


def _check(kind, n, length=0, pen=(4, 6, 2), ad=AD, opts=()):
    """the oracle's records and ops, the kernel's kind, and no more pairs for the retry rung than before the change (HANDED_ON)"""
    what = f"{kind} n={n} length={length} pen={pen} ad={ad} opts={opts}"
    bound = HANDED_ON.get((kind, n, length, pen, ad is not None), 0)
    got, tm = _run(kind, n, length, pen, ad, opts)
    print(f"{what}: main kind {tm.main_kernel_kind}, handed on {tm.n_retried_pairs} (before the change: {bound})")
    assert tm.main_kernel_kind == KIND_DUO, what
    want, want_ops = _want(kind, n, length, pen, ad)
    assert np.array_equal(got.status, want.status), what
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert np.array_equal(a, b), f"{what}: field {f} differs at pairs {np.nonzero(a != b)[0][:8]}"
    assert np.array_equal(_flat_ops(got), want_ops), f"{what}: CIGAR ops differ"
    assert tm.n_retried_pairs <= bound, (what, tm.n_retried_pairs, bound)
    return tm


@pytest.mark.parametrize("length", [260, 1000])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_seed(built, shape, length):
    """first bases that match (the seed is M[0][0], at step 0) and that differ (M[x][0], at step x / g), 1 .. 17 pairs: waves with a
    single running half, with all eight, and a second wave with one"""
    for n in SEED_SIZES:
        _check("first-base", n, length, SHAPES[shape], AD, SHORT)


@pytest.mark.parametrize("ad", [AD, None], ids=["adaptive", "exact"])
@pytest.mark.parametrize("d", ENDS)
def test_sequence_ends(built, d, ad):
    """|m - n| = d, texts longer and shorter than their patterns: the shorter sequence ends first, WF_NEXT's exact path and the
    termination test on the diagonal m - n; 24 pairs of about 300 and about 1 000 bases on three waves, under 4/6/2 and 2/4/2"""
    for pen in ENDS_PEN:
        _check("ends", 24, d, pen, ad, SHORT)


@pytest.mark.parametrize("ad", [AD, None], ids=["adaptive", "exact"])
@pytest.mark.parametrize("kind,n", COPIES)
def test_finish_together_and_in_turn(built, kind, n, ad):
    """copies of one pair: at six pairs per fetch the pairs of a fetch -- both halves of a row among them -- finish in the same step,
    at one pair per fetch they start a step apart and finish on consecutive steps"""
    _check(kind, n, 0, (4, 6, 2), ad, SHORT)


@pytest.mark.parametrize("kind", ["1k5", "1k8"])
@pytest.mark.parametrize("shape", BAND_SHAPES)
def test_band_moves(built, shape, kind):
    """1 kbp pairs that widen, narrow, recentre, park and resume, eight to a wave on 8, 25 and 65 waves; ring depths 4, 3 and 2"""
    for n in BAND_SIZES:
        _check(kind, n, BAND_SEED[kind, n], SHAPES[shape], AD, PINNED)


@pytest.mark.parametrize("n,err", [(520, 5), ("8G+64", 2)])
def test_ragged_lengths(built, n, err):
    """240 .. 1 950 bases in one batch: a freed half row resumes a parked pair, or starts a staged one, of another length.  520 pairs
    at 5 % error, eight to a wave; 8 G + 64 pairs on G waves at 2 % error -- the last 64 are claimed from the queue by whichever wave
    comes first, and bands this narrow leave nothing to who shares a wave"""
    n = 8 * _grid() + 64 if n == "8G+64" else n
    _check("ragged", n, err, (4, 6, 2), AD, PINNED)
    _check("ragged", n, err, (2, 4, 2), AD, PINNED)


def test_out_of_arena_rows(built):
    """96 arena rows a pair (scores up to 190 at 4/6/2): the 2 % pairs fit, the 5 % pairs between them run out of rows and are handed
    on (ST_REDO_ARENA) -- those and no other"""
    n = 520
    tm = _check("rows", n, 0, (4, 6, 2), AD, PINNED + (("packed_arena_bytes", 12 * 1024),))
    assert tm.n_retried_pairs > n // 4
