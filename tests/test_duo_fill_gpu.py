"""GPU: where wfa_duo_kernel puts the next pair into a half row (wfa_duo.hpp; WFA_DUO_FILL in wfa_duo_cfg.hpp).  A half freed by a
pair that finishes -- or runs out of arena rows -- is filled in the finish branch of that score step, parked pairs first, then the
staged pair; restructuring rounds only place what the finish could not.  Nothing but speed may depend on it.

Every test: option duo = 2, wf-adaptive 10/50/1, records and CIGAR ops of EVERY pair against the oracle, and over a poisoned arena
the arena words and pair_meta of the pairs the kernel finished against the 32-bit-ring reference (duo_pk = 0).  The sets of
finished pairs of the two runs may differ only in band hand-ons (ST_REDO_BAND: a widening pair that found its wave's park records
full, which depends on who shares the wave), as in tests/test_duo_claim_gpu.py, whose batches and helpers these tests use.

Cases, at the smallest shapes at which each can go wrong:
  * several halves of a wave finish in the same step with fewer pairs staged than halves freed, so that the fill at the finish leaves
    its loop with halves still free and the round places the rest: 24 G + 3 copies of ONE pair at five and at six pairs per fetch on
    G waves.  The pairs of one fetch start in the same round and, being the same pair, finish in the same step; a wave's first block
    is a fetch of five (six) and one of three (two), so its halves run as a group of five and a group of three from then on.  When
    the three finish, the next fetch of five is staged: three are placed, two stay staged, and no new fetch is stored while a pair
    is staged; when the five finish, two buffers are staged for five free halves.  (What the kernel did is not observable from
    outside; the argument is this one, from the code.)
  * 16, 17 and 24 pairs of 1 kbp whose first eight are one pair: the first wave's halves hold the same pair.  At one pair per fetch
    they start a step apart and finish a step apart, and a grid of ceil(n / 8) waves leaves the first wave nothing to stage
    behind them: these batches check finishes on consecutive steps with the queue dry, not the case above;
  * every ring depth -- a resumed record's row r goes to ring slot (phase + r) mod R, and the finish fills for the NEXT step's
    phase: the six penalty shapes of wfa_launch_duo (R = 2, 3, 4), 1 kbp pairs at 5 % and 8 % error on one wave per CU, three
    rounds of pairs per half row, so that pairs park and resume; most pairs must be finished by this kernel;
  * the queue runs dry at a finish: 1, 7, 8, 9, 65 pairs, and on one wave per CU (G waves) 8 G - 1, 8 G, 8 G + 1 pairs;
  * a staged pair that cannot be aligned here (an empty sequence, a byte outside ACGT) behind finishing pairs: its status and its
    hand-on are recorded and the pair after it takes the half;
  * several pairs per fetch (FP = 5 and 6, duo_short forced): st_mask holds several buffers when a finish consumes one;
  * pairs that end for want of arena rows (packed_arena_bytes small) between pairs that fit: handed on as ST_REDO_ARENA, and the
    pair that takes the half starts its rows at score 0 (its arena words are the reference's).
"""
import functools

import numpy as np
import pytest

from test_duo_claim_gpu import AD, CLASSES, FIELDS, PINNED, ST_REDO_BAND, _canon, _fetch_pairs, _flat_ops, _grid, _pairs, _run

pytestmark = pytest.mark.gpu

ST_EMPTY, ST_REDO_BYTES, ST_REDO_ARENA = 1, 100, 101
# the penalty shapes of wfa_launch_duo (DX : DOE, ring rows R = max of the two)
SHAPES = {"2:4": (4, 6, 2), "1:3": (2, 4, 2), "1:2": (1, 1, 1), "2:3": (4, 4, 2), "2:2": (4, 2, 2), "3:3": (6, 4, 2)}
SHORT = (("duo_short", 2),)
ORACLE_THREADS = 4


def _frozen(data):
    for a in data:
        a.setflags(write=False)
    return tuple(data)


@functools.lru_cache(maxsize=None)
def _batch(kind, n):
    """the batches of this file (built once, read only); offsets may name the same bytes of the blob more than once"""
    import wfa_amd as w
    if kind in CLASSES:
        return _pairs(kind, n)
    if kind.startswith("copies-"):  # n copies of the first pair of a class (its longest pattern: the class's slot and pairs per fetch)
        blob, q_off, q_len, t_off, t_len = _pairs(kind[len("copies-"):], 8)
        one = lambda a: np.full(n, a[0], dtype=a.dtype)
        data = (blob, one(q_off), one(q_len), one(t_off), one(t_len))
        assert _fetch_pairs(data[2], data[4]) == CLASSES[kind[len("copies-"):]][2]
        return _frozen(data)
    if kind == "eight":  # eight copies of one 1 kbp pair, then other pairs
        blob, q_off, q_len, t_off, t_len = (a.copy() for a in _pairs("1k", n))
        q_off[:8], q_len[:8], t_off[:8], t_len[:8] = q_off[0], q_len[0], t_off[0], t_len[0]
        return _frozen((blob, q_off, q_len, t_off, t_len))
    if kind in ("1k5", "1k8"):  # 1 kbp at 5 % / 8 % error
        return _frozen(w.generate_pairs(seed=4100 + n % 89 + (kind == "1k8"), n_pairs=n, length=1000, error_rate=0.08 if kind == "1k8" else 0.05,
                                        n_threads=4))
    if kind == "unalignable":  # every fifth pair cannot be aligned by this kernel: in turn an empty query, an N in the text, an empty text
        blob, q_off, q_len, t_off, t_len = (a.copy() for a in _pairs("1k", n))
        for c, i in enumerate(range(3, n, 5)):
            if c % 3 == 0:
                q_len[i] = 0
            elif c % 3 == 1:
                blob[int(t_off[i]) + int(t_len[i]) // 2] = ord("N")
            else:
                t_len[i] = 0
        return _frozen((blob, q_off, q_len, t_off, t_len))
    if kind == "rows":  # 2 % and 5 % error in turn: under 4/6/2 at most 20 * 8 / 2 = 80 score steps, and about 160
        parts = [w.generate_pairs(seed=4300 + k, n_pairs=(n - k + 1) // 2, length=1000, error_rate=e, n_threads=4) for k, e in enumerate((0.02, 0.05))]
        base = np.array([0, len(parts[0][0])], dtype=np.uint64)
        blob = np.concatenate([parts[0][0], parts[1][0], np.zeros(16, dtype=np.uint8)])
        q_off, t_off = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        q_len, t_len = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        for k, p in enumerate(parts):
            q_off[k::2], q_len[k::2], t_off[k::2], t_len[k::2] = p[1] + base[k], p[2], p[3] + base[k], p[4]
        return _frozen((blob, q_off, q_len, t_off, t_len))
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _want(kind, n, pen):
    """the oracle's records and ops of a batch (computed once, read only)"""
    from oracle import oracle as O
    want = O.align_batch(O.make_params(*pen, global_alignment=True, adaptive=AD), *_batch(kind, n), n_threads=ORACLE_THREADS)
    return want, _flat_ops(want)


def _assert_oracle(got, kind, n, pen, what):
    want, want_ops = _want(kind, n, pen)
    assert np.array_equal(got.status, want.status), what
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert np.array_equal(a, b), f"{what}: field {f} differs at pairs {np.nonzero(a != b)[0][:8]}"
    assert np.array_equal(_flat_ops(got), want_ops), f"{what}: CIGAR ops differ"


def _check(kind, n, pen, opts=(), meta_of=None, min_done=None):
    """the batch through wfa_duo_kernel and through its 32-bit-ring reference, both over a poisoned arena; returns the packed
    run's {pair: pair_meta}"""
    what = f"{kind} n={n} pen={pen} opts={opts}"
    data = _batch(kind, n)
    run = _run(data, pen, 0, opts, meta_of, arena=True)  # (duo_claim = 0: the library's default)
    _assert_oracle(run[0], kind, n, pen, what)
    ref = _run(data, pen, 0, opts, meta_of, arena=True, pk=0)
    _assert_oracle(ref[0], kind, n, pen, what + " (duo_pk=0)")
    (_, tm, metas, slots), (_, tm0, metas0, slots0) = run, ref
    assert metas.keys() == metas0.keys() and len(metas) > 0, what
    done = 0
    for i in metas:
        s, s0 = metas[i][0], metas0[i][0]
        assert s == s0 or {s, s0} == {0, ST_REDO_BAND}, (what, i, metas[i], metas0[i])
        if s != 0 or s0 != 0:  # handed on to another kernel, or not alignable: not the kernel's final state
            continue
        assert metas[i] == metas0[i], (what, i, metas[i], metas0[i])
        assert len(slots[i]) == len(slots0[i]) and np.array_equal(_canon(slots[i]), _canon(slots0[i])), f"{what}: arena of pair {i} differs"
        done += 1
    if meta_of is None:  # (every pair's meta was read: the retry count is the pairs the kernel handed on)
        for t, ms in ((tm, metas), (tm0, metas0)):
            assert t.n_retried_pairs == sum(1 for m in ms.values() if m[0] >= ST_REDO_BYTES), what
    if min_done is not None:
        assert done >= min_done, (what, done, len(metas))
    return metas


@pytest.mark.parametrize("pen", [(4, 6, 2), (2, 4, 2)], ids=["2:4", "1:3"])
@pytest.mark.parametrize("cls", ["short", "short6"])
def test_more_halves_freed_than_pairs_staged(built, cls, pen):
    """24 G + 3 copies of one pair on G waves, five / six pairs per fetch: the pairs of a fetch finish in the same step, in groups that
    the staged buffers do not match (the module's docstring has the schedule) -- fill() at the finish is entered with several free
    halves and leaves with some still free, and with more buffers staged than halves freed.  Every pair is finished by this kernel,
    with one pair_meta and one arena image."""
    n = 24 * _grid() + 3
    sample = np.unique(np.concatenate([np.arange(0, n, 9), np.arange(8 * _grid() - 8, 8 * _grid() + 8), np.arange(n - 16, n)]))
    metas = _check("copies-" + cls, n, pen, PINNED + SHORT, sample, min_done=len(sample))
    assert len(set(metas.values())) == 1 and next(iter(metas.values()))[0] == 0


@pytest.mark.parametrize("n", [16, 17, 24])
def test_first_wave_holds_one_pair_eight_times(built, n):
    """the first wave's eight pairs are one 1 kbp pair (one pair per fetch: they start and finish a step apart), then 8, 9 and 16
    other pairs on a grid of ceil(n / 8) waves: finishes on consecutive steps with nothing left to stage behind them"""
    metas = _check("eight", n, (4, 6, 2), min_done=n)
    assert len({metas[i] for i in range(8)}) == 1
    _check("eight", n, (2, 4, 2), min_done=n)


@pytest.mark.parametrize("kind", ["1k5", "1k8"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_ring_depths(built, shape, kind):
    """every penalty shape, pairs that park and resume: 24 G + 3 pairs on G waves (pair_meta and arena of every ninth pair and of the
    last sixteen); most pairs are finished by this kernel"""
    n = 24 * _grid() + 3
    sample = np.unique(np.concatenate([np.arange(0, n, 9), np.arange(n - 16, n)]))
    _check(kind, n, SHAPES[shape], PINNED, sample, min_done=len(sample) // 2 + 1)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 65])
@pytest.mark.parametrize("cls", list(CLASSES))
def test_queue_dry_small(built, cls, n):
    """fewer pairs than the waves have halves, or a few more: every finish but a handful finds nothing staged"""
    _check(cls, n, (4, 6, 2), SHORT)


@pytest.mark.parametrize("size", ["8G-1", "8G", "8G+1"])
@pytest.mark.parametrize("cls", list(CLASSES))
def test_queue_dry_pinned_grid(built, cls, size):
    """G waves and a pair per half row, but one / exactly / and one more"""
    G = _grid()
    n = {"8G-1": 8 * G - 1, "8G": 8 * G, "8G+1": 8 * G + 1}[size]
    sample = np.unique(np.concatenate([np.arange(0, n, 7), np.arange(n - 16, n)]))
    _check(cls, n, (4, 6, 2), PINNED + SHORT, sample, min_done=len(sample) // 2 + 1)


@pytest.mark.parametrize("cls", ["short", "short6"])
def test_several_pairs_per_fetch(built, cls):
    """FP = 5 and 6, 24 G + 3 pairs on G waves: a finish takes one of several staged buffers, the round or the next finish the others"""
    n = 24 * _grid() + 3
    sample = np.unique(np.concatenate([np.arange(0, n, 9), np.arange(n - 16, n)]))
    _check(cls, n, (4, 6, 2), PINNED + SHORT, sample, min_done=len(sample) // 2 + 1)
    _check(cls, n, (2, 4, 2), PINNED + SHORT, sample, min_done=len(sample) // 2 + 1)


@pytest.mark.parametrize("n", [24, 65, "16G+3"])
def test_unalignable_staged_pair(built, n):
    """every fifth pair is empty or holds a byte outside ACGT: the kernel records its status (and hands the N pair on) where it
    would have started it, at a finish as in a round, and the pair after it takes the half"""
    n = 16 * _grid() + 3 if n == "16G+3" else n
    metas = _check("unalignable", n, (4, 6, 2), PINNED if n > 65 else ())
    for c, i in enumerate(range(3, n, 5)):
        assert metas[i][0] == (ST_REDO_BYTES if c % 3 == 1 else ST_EMPTY), (i, metas[i])
    assert all(metas[i][0] in (0, ST_REDO_BAND) for i in range(n) if i % 5 != 3)


def test_out_of_arena_rows(built):
    """96 arena rows a pair (scores up to 190 at 4/6/2): the 2 % pairs fit, the 5 % pairs run out of rows and are handed on
    (ST_REDO_ARENA), and the halves they leave are filled at that finish"""
    n = 16 * _grid() + 3
    metas = _check("rows", n, (4, 6, 2), PINNED + (("packed_arena_bytes", 12 * 1024),))
    st = np.array([metas[i][0] for i in range(n)])
    assert np.all((st[0::2] == 0) | (st[0::2] == ST_REDO_BAND)) and np.count_nonzero(st[0::2] == 0) > n // 4, np.unique(st[0::2], return_counts=True)
    assert np.count_nonzero(st[1::2] == ST_REDO_ARENA) > n // 4, np.unique(st[1::2], return_counts=True)
