"""GPU: wfahip_score_batch (score only) returns, pair for pair, the status and score of the full path and of the oracle --
global and semi-global, wf-adaptive on and off, every compiled penalty shape and one without an instance, any bytes,
the max_score bound -- and the score kernels, not the full path, do the work."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = [(g, a) for g in (True, False) for a in ((10, 50, 1), None)]


def _aligner(glob, adaptive, pen=(4, 6, 2)):
    import wfa_amd
    al = wfa_amd.New(wfa_amd.Penalties(*pen), wfa_amd.Options(GlobalAlignment=glob), device=0)
    if adaptive is not None:
        assert al.AdaptiveReduction(wfa_amd.AdaptiveReductionOption(*adaptive)) is None
    return al


def _check(al, arrays, glob, adaptive, pen=(4, 6, 2), full=True, max_score=0):
    st, sc = al.score_arrays(*arrays, max_score=max_score)
    want = O.align_batch(O.make_params(*pen, global_alignment=glob, adaptive=adaptive), *arrays, n_threads=16, want_ops=False)
    assert np.array_equal(st, want.status)
    assert np.array_equal(sc, np.where(want.status == 0, want.score, 0).astype(np.uint32))
    if full:
        got = al.align_arrays(*arrays)
        assert np.array_equal(st, got.status) and np.array_equal(sc, np.where(got.status == 0, got.score, 0))
    return st, sc


def _golden_pairs():
    ka = json.load(open(os.path.join(GOLDEN, "known_answers.json")))["vectors"]
    ref = json.load(open(os.path.join(GOLDEN, "ref_test_pairs.json")))
    pairs = [(v["q"].encode(), v["t"].encode()) for v in ka] + [(p["q"].encode(), p["t"].encode()) for p in ref]
    return pairs


@pytest.mark.parametrize("glob,adaptive", MODES)
def test_golden_pairs_match_oracle(glob, adaptive):
    import wfa_amd
    ov = json.load(open(os.path.join(GOLDEN, "oracle_vectors.json")))["results"]
    assert ov  # (the oracle's own golden results are pinned by test_oracle_golden.py; here the oracle is run on the same pairs)
    al = _aligner(glob, adaptive)
    _check(al, wfa_amd.make_blob(*zip(*_golden_pairs())), glob, adaptive)
    wfa_amd.RecycleAligner(al)


def test_readme_text_pair_semi_global():
    al = _aligner(False, (10, 50, 1))
    st, sc = al.ScoreBatch([b"Bioinformatics helps Biology"], [b"We learn bioinformatics to help biologists"])
    assert (int(st[0]), int(sc[0])) == (0, 32)
    assert al.Score(b"Bioinformatics helps Biology", b"We learn bioinformatics to help biologists") == 32
    assert al.last_timing().n_retried_pairs == 1  # (bytes outside ACGT: the full path)


@pytest.mark.parametrize("glob", [True, False])
@pytest.mark.parametrize("adaptive", [(10, 50, 1), None])
@pytest.mark.parametrize("err", [0.05, 0.10, 0.20])
def test_generated_batches(glob, adaptive, err):
    import wfa_amd
    # (4 096 pairs; 1 024 without wf-adaptive, where the oracle's rows stay n + m wide and it takes 30 s for 4 096 at 20 %)
    arrays = wfa_amd.generate_pairs(seed=11, n_pairs=4096 if adaptive else 1024, length=1000, error_rate=err)
    _check(_aligner(glob, adaptive), arrays, glob, adaptive)


def test_short_reads_and_long_pairs():
    import wfa_amd
    _check(_aligner(True, None), wfa_amd.generate_pairs(seed=5, n_pairs=10000, length=150, error_rate=0.02), True, None)
    for glob in (True, False):
        al = _aligner(glob, (10, 50, 1))
        arrays = wfa_amd.generate_pairs(seed=6, n_pairs=3, length=20000, error_rate=0.05)
        al.score_arrays(*arrays)
        assert al.last_timing().n_retried_pairs == 3  # (beyond the score kernels' 2 047 bases)
        _check(al, arrays, glob, (10, 50, 1))


@pytest.mark.parametrize("pen", [(4, 6, 2), (2, 4, 2), (1, 1, 1), (4, 4, 2), (4, 2, 2), (6, 4, 2), (5, 7, 3)])
@pytest.mark.parametrize("glob", [True, False])
def test_penalty_shapes(pen, glob):
    import wfa_amd
    arrays = wfa_amd.generate_pairs(seed=8, n_pairs=512, length=300, error_rate=0.05)
    al = _aligner(glob, (10, 50, 1), pen)
    _check(al, arrays, glob, (10, 50, 1), pen, full=False)
    if pen == (5, 7, 3):  # e / g = 3: no instance -- every pair takes the full path
        assert al.last_timing().n_retried_pairs == 512


@pytest.mark.parametrize("glob", [True, False])
def test_mixed_batch_statuses(glob):
    import wfa_amd
    rng = np.random.default_rng(3)
    qs, ts = [], []
    for i in range(300):
        n = int(rng.integers(1, 900))
        q = bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))
        t = bytearray(q)
        for _ in range(n // 20):
            t[int(rng.integers(0, len(t)))] = int(rng.choice(list(b"ACGT")))
        t = bytes(t)
        kind = i % 6
        if kind == 1:
            q = b""
        elif kind == 2:
            t = b""
        elif kind == 3:
            q = q.lower()
        elif kind == 4:
            t = t[: len(t) // 2] + b"N" + t[len(t) // 2:]
        qs.append(q), ts.append(t)
    al = _aligner(glob, (10, 50, 1))
    st, _ = _check(al, wfa_amd.make_blob(qs, ts), glob, (10, 50, 1))
    assert (st[1::6] == 1).all() and (st[2::6] == 1).all()


@pytest.mark.parametrize("glob", [True, False])
def test_max_score(glob):
    import wfa_amd
    arrays = wfa_amd.generate_pairs(seed=9, n_pairs=2048, length=1000, error_rate=0.10)
    al = _aligner(glob, (10, 50, 1))
    want = O.align_batch(O.make_params(global_alignment=glob, adaptive=(10, 50, 1)), *arrays, n_threads=16, want_ops=False)
    bound = int(np.median(want.score))
    st, sc = al.score_arrays(*arrays, max_score=bound)
    ok = want.score <= bound
    assert ok.any() and (~ok).any()
    assert (st[ok] == 0).all() and np.array_equal(sc[ok], want.score[ok])
    assert (st[~ok] == 8).all() and (sc[~ok] == 0).all()
    st0, sc0 = al.score_arrays(*arrays, max_score=0)
    assert (st0 == 0).all() and np.array_equal(sc0, want.score)


def test_score_kernels_do_the_work():
    import wfa_amd
    al = _aligner(True, (10, 50, 1))
    arrays = wfa_amd.generate_pairs(seed=3, n_pairs=65536, length=1000, error_rate=0.05)
    st, sc = al.score_arrays(*arrays)
    t = al.last_timing()
    assert t.main_kernel_kind == 19 and t.n_retried_pairs <= 0.02 * 65536
    want = O.align_batch(O.make_params(adaptive=(10, 50, 1)), *arrays, n_threads=16, want_ops=False)
    assert np.array_equal(sc, want.score)
    short = wfa_amd.generate_pairs(seed=4, n_pairs=4096, length=300, error_rate=0.02)
    for glob, kind in ((True, 19), (False, 20)):
        al = _aligner(glob, (10, 50, 1))
        al.score_arrays(*short)
        t = al.last_timing()
        assert (t.main_kernel_kind, t.n_retried_pairs, t.arena_bytes) == (kind, 0, 0)
    # launch accounting, (main_kernel_kind, n_launches, n_main_launches) of a call none of whose pairs is handed back: one launch per
    # chunk (wfa_score_kernel, or the wide kernel without wf-adaptive), two under wf-adaptive on the wide kernel (its two phases
    # count as one main launch), one more for the listed long pairs -- the main one where they are most of the call
    import torch
    kbp = wfa_amd.generate_pairs(seed=21, n_pairs=64, length=1000, error_rate=0.05)
    lng = wfa_amd.generate_pairs(seed=22, n_pairs=64, length=2100, error_rate=0.05)
    shift = np.uint64(kbp[0].size)  # the long pairs' blob behind the short pairs'
    both = (np.concatenate([kbp[0], lng[0]]), np.concatenate([kbp[1], lng[1] + shift]), np.concatenate([kbp[2], lng[2]]),
            np.concatenate([kbp[3], lng[3] + shift]), np.concatenate([kbp[4], lng[4]]))
    dev = [torch.from_numpy(a).to("cuda:0") for a in (np.concatenate([kbp[0], np.zeros(64, np.uint8)]), kbp[1].view(np.int64),
                                                       kbp[2].view(np.int32), kbp[3].view(np.int64), kbp[4].view(np.int32))]
    for glob, adaptive, arrays, want in ((True, (10, 50, 1), kbp, (19, 1, 1)), (False, (10, 50, 1), kbp, (20, 2, 1)), (False, None, kbp, (20, 1, 1)),
                                         (True, (10, 50, 1), both, (19, 2, 1)), (True, (10, 50, 1), lng, (23, 1, 1)),
                                         (True, (10, 50, 1), dev, (19, 1, 1)), (False, (10, 50, 1), dev, (20, 2, 1))):
        al = _aligner(glob, adaptive)
        if arrays is dev:
            al.score_tensors(*dev)
        else:
            al.score_arrays(*arrays)
        t = al.last_timing()
        print("launches", glob, adaptive, len(arrays[2]), "retried", t.n_retried_pairs, (t.main_kernel_kind, t.n_launches, t.n_main_launches))
        assert t.n_retried_pairs == 0
        assert (t.main_kernel_kind, t.n_launches, t.n_main_launches) == want
