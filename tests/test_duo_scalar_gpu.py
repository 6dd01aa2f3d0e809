"""GPU: wfa_duo_kernel's wave-uniform state and cold arguments off the score step's path (wfa_duo.hpp; WFA_DUO_SCALAR in wfa_duo_cfg.hpp).
The arguments that only cold code reads -- arena, pair_meta, the redo list, work, chunk_first, queue_head, chunk_n, prepack, g, census -- are
loaded from the kernel-argument segment where they are used; the prefetch's flags and buffer masks are said to be uniform where they are written;
`slow` has a lane mask (slow_m) beside the lane value; the row store's "has the lane a cell" is the OR of the four cell masks; the score index
moves on with one add-with-carry.  Nothing but speed may depend on it.  What can go wrong: a mask that is stale after a pair has parked, resumed,
joined a widening neighbour or started; a store that is skipped or made for a lane without a cell; a score index that moves for a lane that
finished; an argument read from the wrong offset of the segment.

Every test: option duo = 2 (the variable-lanes kernel forced on small batches) over a poisoned arena, records and CIGAR ops of EVERY pair against
the oracle, the kernel's kind (8), and -- run a second time on the 32-bit-ring reference wfa_duo32_kernel (duo_pk = 0), which keeps the form
before -- pair_meta and the arena words of the pairs both runs finished, up to the two bits KERNELS.md 4a names (_canon of
tests/test_duo_claim_gpu.py).  pair_meta's score of a finished pair is the oracle's, exactly.  The two runs may differ in which pairs were handed
on for their band (ST_REDO_BAND depends on who shares a wave), in nothing else.

Cases, at the smallest shapes at which each changed site can go wrong:
  * slow_m -- pairs that reach a sequence end steps before they finish: texts 1 .. 20 bases shorter or longer than their patterns at the end, a
    text 40 bases shorter (a band wider than the 56 diagonals a row holds: handed on, ST_REDO_BAND through the reloaded pair_meta and redo list,
    unless wf-adaptive prunes it back into a row),
    an indel next to the last base; wf-adaptive on and off, 4/6/2 and 2/4/2.  "sharing": 64 pairs, eight to a wave, even pairs 1 kbp at 8 % error
    -- they widen and evict the neighbour in their row -- odd pairs 1 kbp at 1 % error whose text lacks its last 20 bases: about 25 score steps
    to the text's end and 23 more with `slow` set to the end cell on diagonal -20, so that evictions find them with the flag set (parked and
    resumed with it).  Without wf-adaptive the ragged-end pairs' own bands outgrow a half row while the flag is set: the lanes of the half they
    take get the flag from the other half.  (What a wave did is not observable from outside; the argument is this one, from the code.)
  * the store test -- first bases that match and that differ (under 4/6/2 the rows of scores 2 and 6 are empty, the mismatch seed belongs to
    step x / g), 9 pairs of 260 bases, the six penalty shapes, wf-adaptive on and off: every stored word against the reference's arena;
  * si and the finish -- eight copies of one pair (264 bases: six pairs per fetch; 1 kbp: one) finishing in the same step or on consecutive ones;
    pairs that run out of arena rows (96 rows a pair) between pairs that fit;
  * reloaded arguments -- 1 .. 65 pairs at one and at five pairs per fetch; 8 G - 1, 8 G, 8 G + 1 and 24 G + 3 pairs on a pinned grid of G waves
    at five and at six pairs per fetch (the first atomic claim and the guided ones; chunk_n, queue_head and prepack at every fetch); empty and
    non-ACGT pairs staged behind finishing ones (pair_meta and the redo list in fill()); the census instance (census = 1) with the cell counts
    against the oracle's wavefronts.
No debug option reaches wfa_duo_kernel with a work list (KParams::work): the retry rungs that run on lists use other kernels
(wfa_host.hip: rung()), so pair_of()'s list branch is compiled and not run here, as before.

Pairs handed on: a batch with at most eight pairs per wave has the same pairs in a wave in every run (a wave starts with queue entries
[8 w, 8 w + 8)), and policy has not changed: such a batch hands on exactly the pairs the reference kernel hands on, pair for pair, so a wrong
result cannot hide behind the retry rung.  Only the 8 G + 1 and 24 G + 3 batches, whose last pairs go to whichever wave claims them, may differ
in band hand-ons.  (The library before the change handed on the same counts in every case, measured on an MI355X in the same job.)
"""
import functools

import numpy as np
import pytest

from test_duo_claim_gpu import FIELDS, PINNED, ST_REDO_BAND, _canon, _flat_ops, _grid, _pairs
from test_duo_fill_gpu import _batch as _fill_batch
from test_duo_uniform_gpu import _batch as _uni_batch, _blob_of, _bytes, _mutate

pytestmark = pytest.mark.gpu

AD = (10, 50, 1)
SHAPES = {"2:4": (4, 6, 2), "1:3": (2, 4, 2), "1:2": (1, 1, 1), "2:3": (4, 4, 2), "2:2": (4, 2, 2), "3:3": (6, 4, 2)}
SHORT = (("duo_short", 2),)
ST_EMPTY, ST_REDO_BYTES, ST_REDO_ARENA = 1, 100, 101
ORACLE_THREADS = 4
KIND_DUO = 8


@functools.lru_cache(maxsize=None)
def _batch(kind, n):
    """the batches of this file (built once, read only)"""
    import wfa_amd as w
    if kind == "ends":  # about 300 and about 1 000 bases in turn; i % 4: text shorter at its end, longer at its end, 40 shorter, an indel before the last base
        rng = np.random.default_rng(9100 + n)
        qs, ts = [], []
        for i in range(n):
            L = (300, 1000)[i // 4 % 2] + int(rng.integers(0, 24))
            q = list(rng.integers(0, 4, L))
            t = _mutate(rng, q, 0.01 if L < 500 else 0.004)
            d = (1, 3, 7, 12, 20)[i // 8 % 5]
            if i % 4 == 0:
                t = t[:len(t) - d]
            elif i % 4 == 1:
                t = t + [int(x) for x in rng.integers(0, 4, d)]
            elif i % 4 == 2:
                t = t[:len(t) - 40]
            elif i % 8 == 3:
                del t[-2]
            else:
                t.insert(len(t) - 1, (t[-1] + 1) & 3)
            qs.append(_bytes(q)), ts.append(_bytes(t))
        return _blob_of(qs, ts)
    if kind == "sharing":  # even: 1 kbp at 8 % error; odd: 1 kbp at 1 % error, the text without its last 20 bases
        rng = np.random.default_rng(9300 + n)
        qs, ts = [], []
        for i in range(n):
            q = list(rng.integers(0, 4, 1000))
            t = _mutate(rng, q, 0.08 if i % 2 == 0 else 0.01)
            if i % 2 == 1:
                t = t[:len(t) - 20]
            qs.append(_bytes(q)), ts.append(_bytes(t))
        return _blob_of(qs, ts)
    if kind in ("1k", "short", "short6"):  # tests/test_duo_claim_gpu.py: one, five and six pairs per fetch
        return _pairs(kind, n)
    if kind in ("unalignable", "rows"):  # tests/test_duo_fill_gpu.py
        return _fill_batch(kind, n)
    if kind in ("copies-264", "copies-1k"):  # tests/test_duo_uniform_gpu.py
        return _uni_batch(kind, n, 0)
    if kind.startswith("first-base-"):
        return _uni_batch("first-base", n, int(kind[len("first-base-"):]))
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _want(kind, n, pen, ad):
    """the oracle's records and ops of a batch (computed once, read only)"""
    from oracle import oracle as O
    want = O.align_batch(O.make_params(*pen, global_alignment=True, adaptive=ad), *_batch(kind, n), n_threads=ORACLE_THREADS)
    return want, _flat_ops(want)


def _run(kind, n, pen, ad, opts, pk, meta_of):
    """the batch through wfa_duo_kernel (pk = 1) or its 32-bit-ring reference (pk = 0): (result, timing, {pair: pair_meta}, {pair: arena words})"""
    import wfa_amd as w
    from wfa_amd._lib import WfaHipError
    al = w.New(w.Penalties(*pen), w.Options(GlobalAlignment=True), device=0)
    if ad is not None:
        assert al.AdaptiveReduction(w.AdaptiveReductionOption(*ad)) is None
    al.set_option("duo", 2)
    al.set_option("duo_pk", pk)
    al.set_option("arena_poison", 1)
    for k, v in opts:
        al.set_option(k, v)
    got = al.align_arrays(*_batch(kind, n))
    tm = al.last_timing()
    metas, slots = {}, {}
    for i in (range(n) if meta_of is None else meta_of):
        try:
            words, f, meta = al.debug_compact_arena(int(i))
        except WfaHipError:  # (a batch of several chunks: only the last chunk's arena is kept)
            continue
        assert f == 10
        metas[int(i)], slots[int(i)] = meta, words
    al.close()
    return got, tm, metas, slots


def _check(kind, n, pen=(4, 6, 2), ad=AD, opts=(), meta_of=None, fixed_waves=False):
    """oracle, kind, pair_meta and arena words against the reference kernel; fixed_waves: the batch has at most eight pairs per wave, so who shares
    a wave is the same in every run, and the pairs handed on are the reference kernel's, pair for pair.  Returns (the packed run's {pair:
    pair_meta}, its timing)"""
    what = f"{kind} n={n} pen={pen} ad={ad} opts={opts}"
    want, want_ops = _want(kind, n, pen, ad)
    runs = []
    for pk in (1, 0):
        got, tm, metas, slots = _run(kind, n, pen, ad, opts, pk, meta_of)
        print(f"{what} duo_pk={pk}: main kind {tm.main_kernel_kind}, handed on {tm.n_retried_pairs}")
        assert tm.main_kernel_kind == KIND_DUO, what
        assert np.array_equal(got.status, want.status), what
        for f in FIELDS:
            a, b = getattr(got, f), getattr(want, f)
            assert np.array_equal(a, b), f"{what} duo_pk={pk}: field {f} differs at pairs {np.nonzero(a != b)[0][:8]}"
        assert np.array_equal(_flat_ops(got), want_ops), f"{what} duo_pk={pk}: CIGAR ops differ"
        runs.append((tm, metas, slots))
    (tm, metas, slots), (tm0, metas0, slots0) = runs
    assert metas.keys() == metas0.keys() and len(metas) > 0, what
    for i in metas:
        s, s0 = metas[i][0], metas0[i][0]
        assert s == s0 or (not fixed_waves and {s, s0} == {0, ST_REDO_BAND}), (what, i, metas[i], metas0[i])
        if s == 0:  # finished by this kernel: the score in pair_meta is the oracle's, exactly
            assert metas[i][1] == int(want.score[i]), (what, i, metas[i], int(want.score[i]))
        if s != 0 or s0 != 0:  # handed on to another kernel, or not alignable: not the kernel's final state
            continue
        assert metas[i] == metas0[i], (what, i, metas[i], metas0[i])
        assert len(slots[i]) == len(slots0[i]) and np.array_equal(_canon(slots[i]), _canon(slots0[i])), f"{what}: arena of pair {i} differs"
    if meta_of is None:  # (every pair's meta was read: the retry count is at least the pairs this kernel handed on -- a rung may hand a pair on again)
        assert tm.n_retried_pairs >= sum(1 for m in metas.values() if m[0] >= ST_REDO_BYTES), what
    if fixed_waves:
        assert tm.n_retried_pairs == tm0.n_retried_pairs, (what, tm.n_retried_pairs, tm0.n_retried_pairs)
    return metas, tm


@pytest.mark.parametrize("ad", [AD, None], ids=["adaptive", "exact"])
@pytest.mark.parametrize("pen", [(4, 6, 2), (2, 4, 2)], ids=["2:4", "1:3"])
def test_sequence_end_steps_before_the_finish(built, pen, ad):
    """ragged ends, a text 40 bases shorter, an indel before the last base: WF_NEXT's exact path for many steps of a pair, asked for through slow_m"""
    metas, _ = _check("ends", 40, pen, ad, SHORT, fixed_waves=True)
    # (a gap of 40 diagonals: handed on unless wf-adaptive prunes the band back into a row; the others finish here, but for bands that without
    # wf-adaptive outgrow a row too -- with the oracle's result either way, and the same pairs as on the reference kernel)
    st = [metas[i][0] for i in range(40)]
    assert all(s in (0, ST_REDO_BAND) for s in st), st
    assert st[2::4].count(ST_REDO_BAND) >= 5 and st.count(0) >= 20, st


def test_slow_pairs_parked_and_resumed(built):
    """pairs with `slow` set for 23 steps beside pairs that widen into their half: parked and resumed with the flag.  (wf-adaptive on: without it
    the band of a 1 kbp pair at 8 % error outgrows a row and the whole batch is handed on)"""
    metas, _ = _check("sharing", 64, (4, 6, 2), AD, PINNED, fixed_waves=True)
    assert sum(1 for m in metas.values() if m[0] == 0) >= 48, metas


@pytest.mark.parametrize("ad", [AD, None], ids=["adaptive", "exact"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_store_of_early_rows(built, shape, ad):
    """first bases that match and that differ, nine pairs on two waves: empty early rows, the seeds, every stored word against the reference's"""
    metas, _ = _check("first-base-260", 9, SHAPES[shape], ad, SHORT, fixed_waves=True)
    assert sum(1 for m in metas.values() if m[0] == 0) >= 7, metas


@pytest.mark.parametrize("kind", ["copies-264", "copies-1k"])
def test_finish_in_the_same_step(built, kind):
    """eight copies of one pair: one pair_meta, eight times, and the score index of a finished lane does not move"""
    for ad in (AD, None):
        metas, _ = _check(kind, 8, (4, 6, 2), ad, SHORT, fixed_waves=True)
        assert len(set(metas.values())) == 1 and metas[0][0] == 0


def test_out_of_arena_rows_between_pairs_that_fit(built):
    """96 arena rows a pair: the 5 % pairs run out of rows (ST_REDO_ARENA through the reloaded pair_meta and redo list), the 2 % pairs between them
    finish with the oracle's score in pair_meta"""
    n = 64
    metas, tm = _check("rows", n, (4, 6, 2), AD, (("packed_arena_bytes", 12 * 1024),), fixed_waves=True)
    st = np.array([metas[i][0] for i in range(n)])
    assert np.all((st[0::2] == 0) | (st[0::2] == ST_REDO_BAND)) and np.count_nonzero(st[0::2] == 0) > n // 4, st[0::2]
    assert np.all((st[1::2] == ST_REDO_ARENA) | (st[1::2] == ST_REDO_BAND)) and np.count_nonzero(st[1::2] == ST_REDO_ARENA) > n // 4, st[1::2]


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 33, 65])
@pytest.mark.parametrize("cls", ["1k", "short"])
def test_one_to_sixty_five_pairs(built, cls, n):
    """the first blocks of the waves, whole and partial, at one and at five pairs per fetch"""
    _check(cls, n, (4, 6, 2), AD, SHORT, fixed_waves=True)


@pytest.mark.parametrize("size", ["8G-1", "8G", "8G+1", "24G+3"])
@pytest.mark.parametrize("cls", ["short", "short6"])
def test_claims_on_a_pinned_grid(built, cls, size):
    """G waves: the first blocks cover the batch but one pair / exactly / but for one pair that a wave claims with the first atomic; and 16 G + 3
    pairs behind the first blocks, in guided claims; pair_meta and arena of every 29th pair, of the pairs either side of the first claim and
    of the last sixteen"""
    G = _grid()
    n = {"8G-1": 8 * G - 1, "8G": 8 * G, "8G+1": 8 * G + 1, "24G+3": 24 * G + 3}[size]
    sample = np.unique(np.concatenate([np.arange(0, n, 29), np.arange(8 * G - 8, min(n, 8 * G + 8)), np.arange(n - 16, n)]))
    _check(cls, n, (4, 6, 2), AD, PINNED + SHORT, sample, fixed_waves=size in ("8G-1", "8G"))


def test_unalignable_pairs_staged_behind_finishing_ones(built):
    """every fifth pair is empty or holds a byte outside ACGT: fill() writes its status and hands the N pair on"""
    n = 24
    metas, _ = _check("unalignable", n, (4, 6, 2), AD, (), fixed_waves=True)
    for c, i in enumerate(range(3, n, 5)):
        assert metas[i][0] == (ST_REDO_BYTES if c % 3 == 1 else ST_EMPTY), (i, metas[i])
    assert all(metas[i][0] in (0, ST_REDO_BAND) for i in range(n) if i % 5 != 3)


@pytest.mark.parametrize("ad", [AD, None], ids=["adaptive", "exact"])
def test_census_instance(built, ad):
    """wfa_duo_kernel<true, ..> (census = 1): pair_meta's cell count of every finished pair against the words the oracle's wavefronts hold"""
    from oracle import oracle as O
    n, pen = 12, (4, 6, 2)
    metas, _ = _check("ends", n, pen, ad, SHORT + (("census", 1),), fixed_waves=True)
    blob, q_off, q_len, t_off, t_len = _batch("ends", n)
    oa = O.Aligner(O.make_params(*pen, global_alignment=True, adaptive=ad))
    done = 0
    for i in range(n):
        if metas[i][0] != 0:
            continue
        q = bytes(blob[int(q_off[i]):int(q_off[i]) + int(q_len[i])])
        t = bytes(blob[int(t_off[i]):int(t_off[i]) + int(t_len[i])])
        r = oa.align(q, t)
        dump = oa.dump()
        cells = sum(sum(1 for v in raw if v) for c in "MID" for (lo, hi, raw) in dump[c].values())
        assert metas[i][1] == r.score and metas[i][3] == cells, (i, metas[i], r.score, cells)
        done += 1
    assert done >= n // 3
