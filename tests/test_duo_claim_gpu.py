"""GPU: how wfa_duo_kernel's waves claim queue entries (wfa_duo.hpp, prefetch stage of refill; debug option duo_claim).
A wave starts with eight entries of its own ([8 w, 8 w + 8), no atomic), then claims blocks of B fetches from the shared head,
B = clamp((chunk_n - last token) / (2 * grid * FP), 1, duo_claim); duo_claim = 1 claims one fetch per atomic from entry 0 on,
as the kernel did before.  Nothing but speed may depend on it.

Every test: option duo = 2, wf-adaptive 10/50/1, generator pairs, records and CIGARs of EVERY pair against the oracle, and the
pairs the kernel itself finished (pair_meta status OK) against a run with duo_claim = 1 -- the two sets may differ only in
pairs handed on for their band (ST_REDO_BAND: a widening pair that found its wave's park records full, which depends on who
shares the wave), and n_retried_pairs is the number of pairs not in the set.

Read lengths (generator patterns of the lengths in CLASSES, texts a few bases either side): 1 000 .. 1 050 bases, a slot of
more than 128 words, one pair per fetch (FP = 1); 253 .. 300 bases, a slot of 44 words, FP = 5 (the table in
tests/test_seams_gpu.py); 253 .. 272 bases, a slot of 40 words, FP = 6.  With FP > 1 a block is
B * FP entries and the second fetch of a wave's first eight entries is partial.
Batch sizes: 1, 7, 8, 9, 65 pairs (the first blocks cover all of it, partly or exactly); with the grid pinned to G = one wave
per CU, 8 G - 1, 8 G, 8 G + 1 (the first atomic claim) and 8 G + 16 G + 3 pairs (FP = 1: claims of 8 fetches that shrink to 1);
40 003 pairs of 260 .. 300 bases on the full grid (4 096 waves: 2 * grid * FP exceeds what the first blocks leave, every claim is
one fetch, several per wave, and nothing divides chunk_n) and on the pinned grid (claims of 8 fetches of 5 entries, shrinking to 1).
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("score", "tbegin", "tend", "qbegin", "qend", "align_len", "matches", "gaps", "gap_regions", "ops_len")
AD = (10, 50, 1)
ST_REDO_BAND = 103
# class -> (pattern lengths, error rate, pairs per fetch); the texts differ from their patterns by at most round(L * e) bases
# (the longest pattern first: the slot, and with it the pairs per fetch, follows the batch's longest read, in a batch of one pair too)
CLASSES = {"1k": ((1036, 1024, 1012), 0.05, 1), "short": ((290, 276, 262), 0.05, 5), "short6": ((264, 260), 0.03, 6)}
ORACLE_THREADS = 4


def _fetch_pairs(q_len, t_len):
    """pairs per fetch of a batch (wfa_host.hip: seq_words from the longest read; wfa_duo_cfg.hpp: duo_fetch_pairs())"""
    seq_words = (int(max(q_len.max(), t_len.max())) + 15) // 16 + 1
    pw = 4 + 2 * ((seq_words + 1) & ~1)
    return max(1, min(8, 256 // pw))


@functools.lru_cache(maxsize=None)
def _pairs(cls, n):
    """n generator pairs, the class's pattern lengths in turn"""
    import wfa_amd as w
    lengths, err, fp = CLASSES[cls]
    K = len(lengths)
    parts = [w.generate_pairs(seed=1000 + 7 * n + k, n_pairs=(n - k + K - 1) // K, length=L, error_rate=err, n_threads=4)
             for k, L in enumerate(lengths)]
    base = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.uint64)
    blob = np.concatenate([p[0] for p in parts] + [np.zeros(16, dtype=np.uint8)])
    q_off, t_off = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    q_len, t_len = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    for k, p in enumerate(parts):
        q_off[k::K], q_len[k::K], t_off[k::K], t_len[k::K] = p[1] + base[k], p[2], p[3] + base[k], p[4]
    assert _fetch_pairs(q_len, t_len) == fp, (cls, int(q_len.max()), int(t_len.max()))
    data = (blob, q_off, q_len, t_off, t_len)
    for a in data:
        a.setflags(write=False)
    return data


def _flat_ops(r):
    """every pair's ops, pair after pair"""
    ln = r.ops_len.astype(np.int64)
    start = np.concatenate([[0], np.cumsum(ln)[:-1]])
    return r.ops[np.repeat(r.ops_off.astype(np.int64) - start, ln) + np.arange(int(ln.sum()))]


@functools.lru_cache(maxsize=None)
def _want(cls, n, pen):
    """the oracle's records and ops of the batch (computed once, read only)"""
    from oracle import oracle as O
    want = O.align_batch(O.make_params(*pen, global_alignment=True, adaptive=AD), *_pairs(cls, n), n_threads=ORACLE_THREADS)
    return want, _flat_ops(want)


def _run(data, pen, claim, opts=(), meta_of=None, arena=False, pk=1):
    """the batch through wfa_duo_kernel with duo_claim = claim: (result, timing, {pair: pair_meta}, {pair: arena words})"""
    import wfa_amd as w
    from wfa_amd._lib import WfaHipError
    al = w.New(w.Penalties(*pen), w.Options(GlobalAlignment=True), device=0)
    assert al.AdaptiveReduction(w.AdaptiveReductionOption(*AD)) is None
    al.set_option("duo", 2)
    al.set_option("duo_claim", claim)
    al.set_option("duo_pk", pk)
    if arena:
        al.set_option("arena_poison", 1)
    for k, v in opts:
        al.set_option(k, v)
    got = al.align_arrays(*data)
    tm = al.last_timing()
    assert tm.main_kernel_kind == 8
    metas, slots = {}, {}
    for i in (range(len(data[2])) if meta_of is None else meta_of):
        try:
            words, f, meta = al.debug_compact_arena(int(i))
        except WfaHipError:  # (a batch of several chunks: only the last chunk's arena is kept)
            continue
        assert f == 10
        metas[int(i)] = meta
        if arena:
            slots[int(i)] = words
    al.close()
    return got, tm, metas, slots


def _assert_oracle(got, cls, n, pen, what):
    want, want_ops = _want(cls, n, pen)
    assert np.array_equal(got.status, want.status) and not np.any(got.status), what
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert np.array_equal(a, b), f"{what}: field {f} differs at pairs {np.nonzero(a != b)[0][:8]}"
    assert np.array_equal(_flat_ops(got), want_ops), f"{what}: CIGAR ops differ"


def _assert_same_finished(run, ref, what, whole):
    """the pairs the kernel finished itself, this run against the duo_claim = 1 run: apart from band hand-ons the same set"""
    (_, tm, metas, _), (_, tm1, metas1, _) = run, ref
    assert metas.keys() == metas1.keys() and len(metas) > 0, what
    for i in metas:
        s, s1 = metas[i][0], metas1[i][0]
        assert s == s1 or {s, s1} == {0, ST_REDO_BAND}, (what, i, metas[i], metas1[i])
    if whole:  # (every pair's meta was read: the retry count is the pairs the kernel did not finish)
        assert tm.n_retried_pairs == sum(1 for m in metas.values() if m[0] != 0), what
        assert tm1.n_retried_pairs == sum(1 for m in metas1.values() if m[0] != 0), what


def _check(cls, n, pen, claim, opts=(), meta_of=None):
    what = f"{cls} n={n} pen={pen} duo_claim={claim} opts={opts}"
    data = _pairs(cls, n)
    run = _run(data, pen, claim, opts, meta_of)
    _assert_oracle(run[0], cls, n, pen, what)
    ref = _run(data, pen, 1, opts, meta_of)
    _assert_oracle(ref[0], cls, n, pen, what + " (duo_claim=1)")
    _assert_same_finished(run, ref, what, meta_of is None)


def _grid():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


PINNED = (("packed_waves_per_cu", 1),)  # one wave per CU, as tests/test_seams_gpu.py pins the grid


@pytest.mark.parametrize("n", [1, 7, 8, 9, 65])
@pytest.mark.parametrize("cls", list(CLASSES))
def test_first_blocks(built, cls, n):
    """the first blocks cover the whole batch, partly (1, 7, 9, 65 pairs) or exactly (8); the largest also under 2/4/2"""
    _check(cls, n, (4, 6, 2), 8)
    if n == 65:
        _check(cls, n, (2, 4, 2), 8)


@pytest.mark.parametrize("size", ["8G-1", "8G", "8G+1", "24G+3"])
@pytest.mark.parametrize("cls", list(CLASSES))
def test_pinned_grid(built, cls, size):
    """G waves: the first blocks cover the batch but one pair / exactly / but for one pair that one wave claims with the first
    atomic; and 16 G + 3 pairs behind the first blocks: with one pair per fetch claims of 8 fetches that shrink to 1"""
    G = _grid()
    n = {"8G-1": 8 * G - 1, "8G": 8 * G, "8G+1": 8 * G + 1, "24G+3": 8 * G + 8 * G * 2 + 3}[size]
    # (the largest: pair_meta of every third pair, of the pairs either side of the first atomic claim and of the last ones)
    meta_of = None if size != "24G+3" else np.unique(np.concatenate([np.arange(0, n, 3), np.arange(8 * G - 8, 8 * G + 8), np.arange(n - 16, n)]))
    _check(cls, n, (4, 6, 2), 8, PINNED, meta_of)
    if size == "24G+3":
        _check(cls, n, (2, 4, 2), 8, PINNED, meta_of)


@pytest.mark.parametrize("opts", [(), PINNED], ids=["full-grid", "pinned-grid"])
def test_forty_thousand_short_pairs(built, opts):
    """40 003 pairs of 260 .. 300 bases, duo_claim = 8: several blocks per wave, claims that shrink at the end, a chunk_n that
    nothing divides.  (pair_meta of every fifth pair and of the last hundred.)"""
    n = 40003
    meta_of = np.unique(np.concatenate([np.arange(0, n, 5), np.arange(n - 100, n)]))
    _check("short", n, (4, 6, 2), 8, opts, meta_of)


def _canon(words):
    """The arena words as the backtrace reads them.  Which pairs share a wave depends on the order the waves claim the queue,
    and a wave steps WF_NEXT's exact path (rejections near a sequence end) when any of its pairs needs it: the two paths write
    the same offsets and decisions but differ in two bits the backtrace never reads -- fromI next to a set fromX (the exact path
    clears it), and an absent cell (3 on the rejection-free path, 1 on the exact one).  Two runs of the same kernel differ the
    same way; everything else must match byte for byte."""
    w = words.view(np.uint16)
    w = np.where(w == 3, 1, w).astype(np.uint16)
    return np.where((w & 2) != 0, w & ~np.uint16(1), w).astype(np.uint16)


@pytest.mark.parametrize("cls", ["1k", "short"])
def test_claim_values_agree(built, cls):
    """duo_claim = 1, 2, 4 (the default) and 8 on one batch (pinned grid, 8 G + 16 G + 3 pairs): identical records and CIGARs, and over a poisoned
    arena the same arena words in every pair the kernel finished -- duo_claim = 1 and 8 on the packed rings against duo_claim = 1
    on the 32-bit-ring reference (duo_pk = 0)."""
    G = _grid()
    n, pen = 8 * G + 8 * G * 2 + 3, (4, 6, 2)
    data = _pairs(cls, n)
    sample = np.unique(np.concatenate([np.arange(0, n, 9), np.arange(8 * G - 8, 8 * G + 8), np.arange(n - 16, n)]))
    ref = _run(data, pen, 1, PINNED, sample, arena=True, pk=0)
    _assert_oracle(ref[0], cls, n, pen, f"{cls} duo_claim=1 duo_pk=0")
    ref_ops = _flat_ops(ref[0])
    for claim in (1, 2, 4, 8):
        what = f"{cls} duo_claim={claim}"
        run = _run(data, pen, claim, PINNED, sample, arena=claim in (1, 8))
        for f in ("status",) + FIELDS:
            assert np.array_equal(getattr(run[0], f), getattr(ref[0], f)), (what, f)
        assert np.array_equal(_flat_ops(run[0]), ref_ops), what
        _assert_same_finished(run, ref, what, False)
        if claim not in (1, 8):
            continue
        done = 0
        for i, w0 in ref[3].items():
            if ref[2][i][0] != 0 or run[2][i][0] != 0:  # handed on to another kernel: not the kernel's final state
                continue
            assert run[2][i] == ref[2][i], (what, i, run[2][i], ref[2][i])
            assert len(run[3][i]) == len(w0) and np.array_equal(_canon(run[3][i]), _canon(w0)), f"{what}: arena of pair {i} differs"
            done += 1
        assert done >= len(ref[3]) // 2, (what, done)
