"""GPU: global pairs with reads beyond wfa_score_kernel's 2 047 bases are scored by wfa_score_long_kernel (32-bit ring offsets,
the sequences read 2-bit packed from global memory through sliding windows) -- status and score of every pair equal the
oracle's and the full path's, through wfahip_score_batch and wfahip_score_matrix, and the long kernel, not the full path, does
the work: no arena, main_kernel_kind 23 / 24.  Below "score_long_min" (64) long pairs, and for semi-global pairs, routing is as
before."""
import os

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
ADAPT = (10, 50, 1)


def _aligner(glob=True, adaptive=ADAPT, pen=(4, 6, 2), long_min=None, window=None):
    import wfa_amd
    al = wfa_amd.New(wfa_amd.Penalties(*pen), wfa_amd.Options(GlobalAlignment=glob), device=0)
    if adaptive is not None:
        assert al.AdaptiveReduction(wfa_amd.AdaptiveReductionOption(*adaptive)) is None
    if long_min is not None:
        al.set_option("score_long_min", long_min)
    if window is not None:
        al.set_option("score_long_window_words", window)
    return al


def _oracle(arrays, glob=True, adaptive=ADAPT, pen=(4, 6, 2)):
    return O.align_batch(O.make_params(*pen, global_alignment=glob, adaptive=adaptive), *arrays, n_threads=16, want_ops=False)


def _check(al, arrays, glob=True, adaptive=ADAPT, pen=(4, 6, 2), full=False, max_score=0):
    st, sc = al.score_arrays(*arrays, max_score=max_score)
    t = al.last_timing()
    want = _oracle(arrays, glob, adaptive, pen)
    assert np.array_equal(st, want.status)
    assert np.array_equal(sc, np.where(want.status == 0, want.score, 0).astype(np.uint32))
    if full:
        got = al.align_arrays(*arrays)
        assert np.array_equal(st, got.status) and np.array_equal(sc, np.where(got.status == 0, got.score, 0))
    return st, sc, t


def _seqs(arrays):
    blob, q_off, q_len, t_off, t_len = arrays
    qs = [bytes(blob[int(o):int(o) + int(n)]) for o, n in zip(q_off, q_len)]
    ts = [bytes(blob[int(o):int(o) + int(n)]) for o, n in zip(t_off, t_len)]
    return qs, ts


def _mutate(rng, s, rate):
    out = bytearray()
    for c in s:
        r = rng.random()
        if r < rate / 3:
            out.append(b"ACGT"[rng.integers(4)])  # substitution
        elif r < 2 * rate / 3:
            continue  # deletion
        elif r < rate:
            out += bytes([c, b"ACGT"[rng.integers(4)]])  # insertion
        else:
            out.append(c)
    return bytes(out)


def _rand(rng, n):
    return bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))


def _families(seed, n_fam, k, length, rate):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_fam):
        anc = _rand(rng, length)
        out += [_mutate(rng, anc, rate) for _ in range(k)]
    return out


def test_long_kernel_does_the_work():
    """256 generated pairs of 20 kbp @5 %, seed 31, wf-adaptive 10/50/1: wfa_score_long_kernel scores them, nothing is allocated
    for a backtrace, and at most 2 % of the pairs may have gone to the full path.  The inputs allow it: the oracle alone, run on
    these 256 pairs on the CPU (Aligner.wavefront(0, s) of every score), never holds an M row wider than 69 diagonals (median of
    the pairs' widest rows: 52), so 0 % of the pairs come near the ring's 248."""
    import wfa_amd
    arrays = wfa_amd.generate_pairs(seed=31, n_pairs=256, length=20000, error_rate=0.05)
    al = _aligner()
    st, sc, t = _check(al, arrays)
    print("kind", t.main_kernel_kind, "retried", t.n_retried_pairs, "arena", t.arena_bytes, "kernel_ms", t.kernel_ms)
    assert (st == 0).all()
    assert t.main_kernel_kind == 23
    assert t.arena_bytes == 0
    assert t.n_retried_pairs <= 0.02 * 256


def test_lengths_around_the_hand_over():
    import wfa_amd
    rng = np.random.default_rng(5)
    qs, ts = [], []
    for ln in range(2040, 2061):  # both sides of SCORE_MAX_LEN = 2 047, either sequence the longer one
        for v in range(4):
            q = _rand(rng, ln)
            t = _mutate(rng, q, 0.04)
            qs.append(q if v & 1 else t), ts.append(t if v & 1 else q)
    for _ in range(64):  # a long query against a short target and the reverse: a pure-gap tail
        q = _rand(rng, 5000)
        qs.append(q), ts.append(_mutate(rng, q[:1500], 0.03))
        t = _rand(rng, 5000)
        qs.append(_mutate(rng, t[:1500], 0.03)), ts.append(t)
    arrays = wfa_amd.make_blob(qs, ts)
    n_long = sum(1 for q, t in zip(qs, ts) if max(len(q), len(t)) > 2047)
    assert n_long >= 128 and n_long < len(qs)
    al = _aligner()
    _, _, t = _check(al, arrays, full=True)
    # (the timing read inside _check is the score call's: the pure-gap tails may leave the ring and be handed on, the rest may not)
    assert t.main_kernel_kind == 23 and t.n_retried_pairs <= 128
    # one, two and three long pairs: under the gate they take the full path, with the gate at 1 the long kernel
    longs = [i for i in range(len(qs)) if max(len(qs[i]), len(ts[i])) > 2047 and len(qs[i]) < 4000 and len(ts[i]) < 4000]
    for k in (1, 2, 3):
        sub = wfa_amd.make_blob([qs[i] for i in longs[:k]], [ts[i] for i in longs[:k]])
        _, _, t = _check(_aligner(), sub)
        assert t.n_retried_pairs == k and t.main_kernel_kind != 23
        _, _, t = _check(_aligner(long_min=1), sub)
        assert (t.n_retried_pairs, t.arena_bytes, t.main_kernel_kind) == (0, 0, 23)


@pytest.mark.parametrize("err", [0.05, 0.10, 0.20])
def test_error_rates_with_wf_adaptive(err):
    import wfa_amd
    arrays = wfa_amd.generate_pairs(seed=32, n_pairs=64, length=20000, error_rate=err)
    _, _, t = _check(_aligner(), arrays, full=err == 0.05)
    assert t.main_kernel_kind == 23


def test_wf_adaptive_off():
    import wfa_amd
    # 2 200 bases @1 %: 22 edits of at most o + e = 8 each bound the score by 176, and a row of score s spans at most
    # 2 (s - o) / e + 1 = 171 diagonals: inside the ring, nothing is handed on
    arrays = wfa_amd.generate_pairs(seed=33, n_pairs=64, length=2200, error_rate=0.01)
    _, _, t = _check(_aligner(adaptive=None), arrays, adaptive=None, full=True)
    assert (t.main_kernel_kind, t.n_retried_pairs, t.arena_bytes) == (23, 0, 0)
    # 3 000 bases @5 %: 150 edits of at least 4 each, a score of 600 or more, rows growing by a diagonal on either side per
    # e = 2 of score: every pair's band passes 248 diagonals long before it ends and comes back through the full path
    arrays = wfa_amd.generate_pairs(seed=34, n_pairs=64, length=3000, error_rate=0.05)
    _, _, t = _check(_aligner(adaptive=None), arrays, adaptive=None)
    assert t.n_retried_pairs == 64 and t.arena_bytes > 0


def test_windows():
    import wfa_amd
    rng = np.random.default_rng(7)
    same = _rand(rng, 21000)  # ONE match run through every window
    read = _rand(rng, 21000)
    qs = [same, read, read[:9000] + read[12000:]]
    ts = [same, read[:9000] + read[12000:], read]  # a 3 kbp deletion / insertion in the middle: the band jumps
    g_qs, g_ts = _seqs(wfa_amd.generate_pairs(seed=35, n_pairs=12, length=20000, error_rate=0.05))
    arrays = wfa_amd.make_blob(qs + g_qs, ts + g_ts)
    want = _oracle(arrays)
    assert want.score[0] == 0
    got = []
    for window in (256, 64, 16, 1024):
        al = _aligner(long_min=1, window=window)
        st, sc = al.score_arrays(*arrays)
        t = al.last_timing()
        assert np.array_equal(st, want.status) and np.array_equal(sc, want.score), window
        assert t.main_kernel_kind == 23
        got.append((st, sc, t.n_retried_pairs))
    for g in got[1:]:  # the window decides speed only: the same pairs finished on the kernel, with the same results
        assert np.array_equal(g[0], got[0][0]) and np.array_equal(g[1], got[0][1]) and g[2] == got[0][2]


@pytest.mark.parametrize("pen", [(4, 6, 2), (2, 4, 2), (1, 1, 1), (6, 4, 2), (5, 7, 3)])
def test_penalty_shapes(pen):
    import wfa_amd
    arrays = wfa_amd.generate_pairs(seed=36, n_pairs=64, length=5000, error_rate=0.05)
    _, _, t = _check(_aligner(pen=pen), arrays, pen=pen)
    if pen == (5, 7, 3):  # e / g = 3: no instance -- every pair takes the full path
        assert t.n_retried_pairs == 64 and t.main_kernel_kind != 23
    else:
        assert t.main_kernel_kind == 23 and t.n_retried_pairs <= 1 and (t.arena_bytes == 0) == (t.n_retried_pairs == 0)


def test_max_score():
    import wfa_amd
    arrays = wfa_amd.generate_pairs(seed=37, n_pairs=128, length=20000, error_rate=0.05)
    al = _aligner()
    want = _oracle(arrays)
    bound = int(np.median(want.score))
    st, sc = al.score_arrays(*arrays, max_score=bound)
    assert al.last_timing().main_kernel_kind == 23
    ok = want.score <= bound
    assert ok.any() and (~ok).any()
    assert (st[ok] == 0).all() and np.array_equal(sc[ok], want.score[ok])
    assert (st[~ok] == 8).all() and (sc[~ok] == 0).all()
    st0, sc0 = al.score_arrays(*arrays, max_score=0)
    assert (st0 == 0).all() and np.array_equal(sc0, want.score)


def test_mixed_batch():
    import wfa_amd
    s_qs, s_ts = _seqs(wfa_amd.generate_pairs(seed=38, n_pairs=4096, length=1000, error_rate=0.05))
    l_qs, l_ts = _seqs(wfa_amd.generate_pairs(seed=39, n_pairs=128, length=20000, error_rate=0.05))
    al = _aligner()
    al.score_arrays(*wfa_amd.make_blob(s_qs, s_ts))
    band_short = al.last_timing().n_retried_pairs  # (band hand-backs of the two halves on their own: a pair's own property)
    al.score_arrays(*wfa_amd.make_blob(l_qs, l_ts))
    band_long = al.last_timing().n_retried_pairs
    assert al.last_timing().main_kernel_kind == 23
    qs, ts = list(s_qs), list(s_ts)
    for j in range(128):  # the long pairs scattered among the short ones
        qs.insert(j * 33 + 7, l_qs[j]), ts.insert(j * 33 + 7, l_ts[j])
    odd = [(b"", s_ts[0]), (l_qs[0], b""), (s_qs[1].lower(), s_ts[1]), (l_qs[1], l_ts[1].lower()),
           (s_qs[2][:500] + b"N" + s_qs[2][500:], s_ts[2]), (l_qs[2][:9000] + b"N" + l_qs[2][9000:], l_ts[2]), (l_qs[3], l_ts[3][:-1] + b"N")]
    for j, (q, t) in enumerate(odd):
        qs.insert(j * 500 + 3, q), ts.insert(j * 500 + 3, t)
    st, sc, t = _check(al, wfa_amd.make_blob(qs, ts), full=True)
    assert (st == 1).sum() == 2
    assert t.main_kernel_kind == 19  # (wfa_score_kernel took 4 096 pairs, the long kernel 128)
    assert t.n_retried_pairs == band_short + band_long + 5  # the five pairs with a byte outside ACGT, and the band hand-backs


def test_semi_global_long_pairs_are_unchanged():
    import wfa_amd
    arrays = wfa_amd.generate_pairs(seed=40, n_pairs=64, length=20000, error_rate=0.05)
    _, _, t = _check(_aligner(glob=False), arrays, glob=False)
    assert t.n_retried_pairs == 64 and t.main_kernel_kind not in (23, 24)


def _expand(qs, ts):
    import wfa_amd
    return wfa_amd.make_blob([q for q in qs for _ in ts], [t for _ in qs for t in ts])


def _related(seed, n_fam, k, length, fam_rate, rate):
    """n_fam families of k reads whose ancestors descend from one root: reads of different families still align."""
    rng = np.random.default_rng(seed)
    root = _rand(rng, length)
    out = []
    for _ in range(n_fam):
        anc = _mutate(rng, root, fam_rate)
        out += [_mutate(rng, anc, rate) for _ in range(k)]
    return out


def test_matrix_all_against_all():
    """24 reads of 6 kbp in four families, all against all: 576 cells, every one of them long, none for the full path.  The
    families' ancestors are 4 % from a common root and the reads 2 % from their ancestor (reads of different families ~12 %
    apart): the oracle alone, run on the 576 cells on the CPU, never holds an M row wider than 95 diagonals.  (Four UNRELATED
    families do not allow the arena-free condition: the oracle's rows pass 240 diagonals in 20 to 40 of their 576 cells.)"""
    reads = _related(41, 4, 6, 6000, 0.04, 0.02)
    al = _aligner()
    st, sc = al.ScoreMatrix(reads)
    t = al.last_timing()
    print("kind", t.main_kernel_kind, "retried", t.n_retried_pairs, "arena", t.arena_bytes)
    arrays = _expand(reads, reads)
    want = _oracle(arrays)
    assert np.array_equal(st.ravel(), want.status) and np.array_equal(sc.ravel(), want.score)
    bst, bsc = al.score_arrays(*arrays)
    assert np.array_equal(st.ravel(), bst) and np.array_equal(sc.ravel(), bsc)
    assert al.last_timing().n_retried_pairs == t.n_retried_pairs  # (the same kernel's decisions, cell by cell)
    assert t.main_kernel_kind == 24 and t.arena_bytes == 0


def test_matrix_mixed_tiles_and_stride():
    import wfa_amd
    rng = np.random.default_rng(9)
    fam = _families(43, 1, 10, 6000, 0.04)
    short = _families(44, 1, 8, 1000, 0.05)
    qs = fam[:5] + short[:4] + [b"", fam[5][:3000] + b"N" + fam[5][3000:]]
    ts = fam[5:] + short[4:] + [short[0][:400] + b"N", b"", _rand(rng, 2048)]
    al = _aligner()
    arrays = _expand(qs, ts)
    want = _oracle(arrays)
    wst = want.status.reshape(len(qs), len(ts))
    wsc = np.where(want.status == 0, want.score, 0).astype(np.uint32).reshape(len(qs), len(ts))
    st, sc = al.ScoreMatrix(qs, ts)
    t = al.last_timing()
    assert np.array_equal(st, wst) and np.array_equal(sc, wsc)
    # the full path takes the 20 non-empty cells of the two reads with an N, and whatever band the kernels hand back (a 1 kbp read against
    # a 6 kbp one is mostly gap); the 25 cells within the 6 kbp family and the 16 within the 1 kbp one stay on the kernels
    assert t.main_kernel_kind in (21, 24) and 20 <= t.n_retried_pairs <= len(qs) * len(ts) - 5 * 5 - 4 * 4
    retried = t.n_retried_pairs
    al.set_option("matrix_tile_cells", 7)  # tiles of 1 x 7: rows and columns split, tiles with and without long cells
    st, sc = al.ScoreMatrix(qs, ts)
    assert np.array_equal(st, wst) and np.array_equal(sc, wsc) and al.last_timing().n_retried_pairs == retried
    # a window of a larger sentinel-filled matrix
    big_st, big_sc = np.full((20, 40), -5, np.int32), np.full((20, 40), 0xDEADBEEF, np.uint32)
    blob, off, ln, _, _ = wfa_amd.make_blob(qs + ts, [b""] * (len(qs) + len(ts)))
    nq, nt = len(qs), len(ts)
    al.score_matrix_arrays(blob, off[:nq], ln[:nq], off[nq:], ln[nq:], out=(big_st[3:3 + nq, 7:7 + nt], big_sc[3:3 + nq, 7:7 + nt]))
    assert np.array_equal(big_st[3:3 + nq, 7:7 + nt], wst) and np.array_equal(big_sc[3:3 + nq, 7:7 + nt], wsc)
    mask = np.ones((20, 40), bool)
    mask[3:3 + nq, 7:7 + nt] = False
    assert (big_st[mask] == -5).all() and (big_sc[mask] == 0xDEADBEEF).all()
    al.set_option("matrix_tile_cells", 0)
    # under the gate (one long read against a few short ones) the cells take the full path, as before
    st, sc = al.ScoreMatrix(fam[:1], short[:3])
    assert al.last_timing().n_retried_pairs == 3 and al.last_timing().main_kernel_kind == 21


def test_score_long_min_is_a_debug_key(built):
    import wfa_amd as w
    from wfa_amd import _lib as L
    al = w.New()
    lib = L.lib()
    saved = os.environ.pop("WFAHIP_DEBUG", None)
    try:
        for key in (b"score_long_min", b"score_long_window_words"):
            assert lib.wfahip_set_option(al._ctx, key, 1) == L.ERR_UNSUPPORTED, key
            assert b"WFAHIP_DEBUG" in lib.wfahip_last_error(al._ctx)
        os.environ["WFAHIP_DEBUG"] = "0"
        assert lib.wfahip_set_option(al._ctx, b"score_long_min", 1) == L.ERR_UNSUPPORTED
        os.environ["WFAHIP_DEBUG"] = "1"
        assert lib.wfahip_set_option(al._ctx, b"score_long_min", 1) == L.OK
        assert lib.wfahip_set_option(al._ctx, b"score_long_window_words", 64) == L.OK
    finally:
        if saved is None:
            os.environ.pop("WFAHIP_DEBUG", None)
        else:
            os.environ["WFAHIP_DEBUG"] = saved
    al.close()
