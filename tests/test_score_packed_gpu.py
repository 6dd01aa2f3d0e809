"""GPU: wfahip_score_batch_packed (score only on 2-bit packed input) returns, pair for pair, the status and score of
wfahip_score_batch on the unpacked bytes and of the oracle -- global and semi-global, wf-adaptive on and off, every penalty route,
the kernels' length limits, the bound -- with the same kernels doing the work (main_kernel_kind, n_retried_pairs), offsets that
repeat and come in any order, and nothing beyond a sequence's last base read as sequence."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
ADAPT = (10, 50, 1)
MODES = [(True, ADAPT), (True, None), (False, ADAPT), (False, None)]  # (global alignment, wf-adaptive)
MAX_SEQ_LEN = (1 << 29) - 1
PAIR_EMPTY, PAIR_TOO_LONG, PAIR_OVER_MAX = 1, 2, 8


def _aligner(glob=True, adaptive=ADAPT, pen=(4, 6, 2), long_min=None):
    import wfa_amd
    al = wfa_amd.New(wfa_amd.Penalties(*pen), wfa_amd.Options(GlobalAlignment=glob), device=0)
    if adaptive is not None:
        assert al.AdaptiveReduction(wfa_amd.AdaptiveReductionOption(*adaptive)) is None
    if long_min is not None:
        al.set_option("score_long_min", long_min)
    return al


def _oracle(arrays, glob, adaptive, pen=(4, 6, 2)):
    return O.align_batch(O.make_params(*pen, global_alignment=glob, adaptive=adaptive), *arrays, n_threads=16, want_ops=False)


def _expected(want, max_score=0):
    st = want.status.astype(np.int32).copy()
    if max_score:
        st[(want.status == 0) & (want.score > max_score)] = PAIR_OVER_MAX
    return st, np.where(st == 0, want.score, 0).astype(np.uint32)


def _pack(arrays):
    """(packed, q_woff, q_len, t_woff, t_len) of a byte batch, through wfahip_pack_pairs"""
    import wfa_amd
    packed, qw, tw = wfa_amd.pack_pairs(*arrays)
    return packed, qw, arrays[2], tw, arrays[4]


def _three(al, arrays, pk, want, max_score=0):
    """the three sides of every comparison: the packed entry, the byte entry, the oracle -- and the two entries' routing"""
    st_b, sc_b = al.score_arrays(*arrays, max_score=max_score)
    tb = al.last_timing()
    st_p, sc_p = al.score_arrays_packed(*pk, max_score=max_score)
    tp = al.last_timing()
    print("byte: kind", tb.main_kernel_kind, "retried", tb.n_retried_pairs, "arena", tb.arena_bytes, "| packed: kind", tp.main_kernel_kind,
          "retried", tp.n_retried_pairs, "arena", tp.arena_bytes)
    st_o, sc_o = _expected(want, max_score)
    assert np.array_equal(st_p, st_b) and np.array_equal(sc_p, sc_b)
    assert np.array_equal(st_p, st_o) and np.array_equal(sc_p, sc_o)
    assert tp.main_kernel_kind == tb.main_kernel_kind
    assert tp.n_retried_pairs == tb.n_retried_pairs
    if tb.arena_bytes == 0:
        assert tp.arena_bytes == 0
    return st_p, sc_p, tp


def _rand(rng, n):
    return bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))


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


def _pair_of(rng, length, rate):
    """a pair whose longer read has exactly `length` bases"""
    q = _rand(rng, length)
    t = _mutate(rng, q, rate)[:length] or q[:1]
    return (q, t) if rng.random() < 0.5 else (t, q)


def _pack_seq(s):
    """one sequence as wfahip_pack_pairs writes it: 16 bases per word, code (ascii >> 1) & 3, then the pad word"""
    a = np.frombuffer(s, dtype=np.uint8)
    nw = (len(a) + 15) // 16
    codes = np.zeros(nw * 16, dtype=np.uint64)
    codes[:len(a)] = (a >> 1) & 3
    words = (codes.reshape(nw, 16) << (2 * np.arange(16, dtype=np.uint64))).sum(axis=1).astype(np.uint32)
    return np.concatenate([words, np.zeros(1, np.uint32)])


def _lay(seqs, gap=0, fill=0):
    """the sequences packed one after another, `gap` words of `fill` between them: (packed, word offset of each)"""
    parts, offs, pos = [], [], 0
    for s in seqs:
        w = _pack_seq(s)
        offs.append(pos), parts.append(w), parts.append(np.full(gap, fill, np.uint32))
        pos += len(w) + gap
    return np.concatenate(parts + [np.zeros(1, np.uint32)]), np.array(offs, dtype=np.uint64)


def test_word_boundaries():
    import wfa_amd
    rng = np.random.default_rng(11)
    qs, ts = [], []
    for ln in (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257):
        q = _rand(rng, ln)
        sub = bytearray(q)  # the same length, a handful of substitutions
        for _ in range(min(3, ln)):
            sub[rng.integers(ln)] = b"ACGT"[rng.integers(4)]
        qs.append(q), ts.append(bytes(sub))
        qs.append(q), ts.append(_mutate(rng, q, 0.06) or b"A")  # ... and a handful of edits of any kind
        qs.append(_mutate(rng, q, 0.06) or b"C"), ts.append(q)
    for n, m in ((1, 40), (17, 300), (300, 16), (16, 33), (257, 64), (33, 1)):
        long_ = _rand(rng, max(n, m))
        start = int(rng.integers(0, max(n, m) - min(n, m) + 1))
        short = _mutate(rng, long_[start:start + min(n, m)], 0.05)[:min(n, m)]
        short = short + _rand(rng, min(n, m) - len(short))
        qs.append(long_ if n >= m else short), ts.append(short if n >= m else long_)
        assert (len(qs[-1]), len(ts[-1])) == (n, m)
    arrays = wfa_amd.make_blob(qs, ts)
    pk = _pack(arrays)
    for glob, adaptive in MODES:
        _three(_aligner(glob, adaptive), arrays, pk, _oracle(arrays, glob, adaptive))


def test_length_limits():
    import wfa_amd
    rng = np.random.default_rng(12)
    by_len = {ln: [_pair_of(rng, ln, 0.02) for _ in range(8)] for ln in (2046, 2047, 2048, 2049)}

    def batch(lens):
        ps = [p for ln in lens for p in by_len[ln]]
        arrays = wfa_amd.make_blob([p[0] for p in ps], [p[1] for p in ps])
        return arrays, _pack(arrays)

    short, long_, both = batch((2046, 2047)), batch((2048, 2049)), batch((2046, 2047, 2048, 2049))
    # global: 2 047 bases run on wfa_score_kernel, 2 048 on the long kernel (gate at one pair)
    for adaptive in (ADAPT, None):
        al = _aligner(True, adaptive, long_min=1)
        _, _, t = _three(al, *short, _oracle(short[0], True, adaptive))
        assert t.main_kernel_kind == 19
        _, _, t = _three(al, *long_, _oracle(long_[0], True, adaptive))
        assert t.main_kernel_kind == 23  # (every pair is long: the short launch is skipped)
        _, _, t = _three(al, *both, _oracle(both[0], True, adaptive))
        assert t.main_kernel_kind == 19  # (as many pairs on either kernel: the long one did not take more)
        if adaptive is not None:
            assert t.n_retried_pairs == 0 and t.arena_bytes == 0  # (2 % under wf-adaptive: no band near 248 diagonals)
    # semi-global: 2 048 bases and up take the full path
    al = _aligner(False, ADAPT, long_min=1)
    _, _, t = _three(al, *short, _oracle(short[0], False, ADAPT))
    assert t.main_kernel_kind == 20 and t.n_retried_pairs < 16
    short_retried = t.n_retried_pairs
    _, _, t = _three(al, *both, _oracle(both[0], False, ADAPT))
    assert t.main_kernel_kind == 20 and t.n_retried_pairs == 16 + short_retried
    # three global pairs of 20 000 bases under the default gate (64): all three are handed back and gathered
    ps = [_pair_of(rng, 20000, 0.02) for _ in range(3)]
    arrays = wfa_amd.make_blob([p[0] for p in ps], [p[1] for p in ps])
    al = _aligner(True, ADAPT)
    _, _, t = _three(al, arrays, _pack(arrays), _oracle(arrays, True, ADAPT))
    assert t.n_retried_pairs == 3


@pytest.mark.parametrize("pen", [(4, 6, 2), (2, 4, 2), (1, 1, 1), (4, 4, 2), (6, 4, 2), (5, 7, 3)])
def test_penalty_routes(pen):
    import wfa_amd
    arrays = wfa_amd.generate_pairs(seed=21, n_pairs=512, length=300, error_rate=0.05)
    pk = _pack(arrays)
    for glob in (True, False):
        _, _, t = _three(_aligner(glob, ADAPT, pen), arrays, pk, _oracle(arrays, glob, ADAPT, pen))
        if pen == (5, 7, 3):  # no instance: every pair goes through the gather and the packed full path
            assert t.n_retried_pairs == 512
        else:  # (an instance takes the batch; the few pairs it may hand back are the byte entry's, checked above)
            assert t.main_kernel_kind == (19 if glob else 20) and t.n_retried_pairs <= 10


def test_band_the_ring_cannot_hold():
    import wfa_amd
    rng = np.random.default_rng(14)
    blob, q_off, q_len, t_off, t_len = wfa_amd.generate_pairs(seed=22, n_pairs=200, length=300, error_rate=0.05)
    qs = [bytes(blob[int(o):int(o) + int(n)]) for o, n in zip(q_off, q_len)]
    ts = [bytes(blob[int(o):int(o) + int(n)]) for o, n in zip(t_off, t_len)]
    for at in (3, 77, 150, 199):  # two unrelated reads: the band outgrows the ring's 248 diagonals long before they end
        qs.insert(at, _rand(rng, 700)), ts.insert(at, _rand(rng, 700))
    arrays = wfa_amd.make_blob(qs, ts)
    _, _, t = _three(_aligner(True, None), arrays, _pack(arrays), _oracle(arrays, True, None))
    assert t.main_kernel_kind == 19 and t.n_retried_pairs >= 4


@pytest.mark.parametrize("pen", [(4, 6, 2), (5, 7, 3)])  # (5, 7, 3): no instance, every pair -- these too -- is handed to the full path
@pytest.mark.parametrize("glob", [True, False])
def test_per_pair_statuses(glob, pen):
    import wfa_amd
    from wfa_amd import _lib
    rng = np.random.default_rng(15)
    qs = [_rand(rng, 120) for _ in range(8)]
    ts = [_mutate(rng, q, 0.05) for q in qs]
    qs[2], ts[5] = b"", b""  # an empty query, an empty target
    blob, q_off, q_len, t_off, t_len = wfa_amd.make_blob(qs, ts)
    packed, offs = _lay(qs + ts)
    qw, tw = offs[:8].copy(), offs[8:].copy()
    q_len = q_len.copy()
    q_len[6] = MAX_SEQ_LEN + 1  # too long: its offset is never looked at
    qw[6] = np.uint64(1 << 40)
    tw[2] = np.uint64(1 << 41)  # the empty query's target: not looked at either
    arrays = (blob, q_off, q_len, t_off, t_len)
    al = _aligner(glob, ADAPT, pen)
    st, _, t = _three(al, arrays, (packed, qw, q_len, tw, t_len), _oracle(arrays, glob, ADAPT, pen))
    if pen == (5, 7, 3):
        assert t.n_retried_pairs == 8
    assert st[2] == PAIR_EMPTY and st[5] == PAIR_EMPTY and st[6] == PAIR_TOO_LONG and (np.delete(st, (2, 5, 6)) == 0).all()

    # whole-call errors: a non-empty pair whose words end past n_words; a hostile offset.  out stays zeroed.
    def call(qw_, n_words):
        out = _lib.Scores()
        out.n = 99
        prm = al._params()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = _lib.lib().wfahip_score_batch_packed(al._ctx, C.byref(prm), vp(packed), n_words, vp(qw_), vp(q_len), vp(tw), vp(t_len), 8, 0,
                                                  C.byref(out))
        return rc, out
    n_words = int(tw[7]) + (int(t_len[7]) + 15) // 16 + 1  # the last sequence's words, pad word included
    rc, out = call(qw, n_words)
    assert rc == 0 and out.n == 8
    _lib.lib().wfahip_scores_free(C.byref(out))
    rc, out = call(qw, n_words - 1)  # (its pad word is past the end)
    assert rc == _lib.ERR_BAD_ARG and out.n == 0 and not out.status and not out.score
    hostile = qw.copy()
    hostile[0] = np.uint64(1 << 63)
    rc, out = call(hostile, n_words)
    assert rc == _lib.ERR_BAD_ARG and out.n == 0 and not out.status and not out.score


def test_the_bound():
    import wfa_amd
    rng = np.random.default_rng(16)
    qs, ts = [], []
    for _ in range(256):
        q = _rand(rng, int(rng.integers(150, 1001)))
        qs.append(q), ts.append(_mutate(rng, q, float(rng.uniform(0.02, 0.15))))
    arrays = wfa_amd.make_blob(qs, ts)
    pk = _pack(arrays)
    for glob, adaptive in MODES:
        want = _oracle(arrays, glob, adaptive)
        assert (want.status == 0).all()
        top = int(want.score.max())
        al = _aligner(glob, adaptive)
        for bound in (0, 1, int(np.median(want.score)), top, top - 1):
            st, _, _ = _three(al, arrays, pk, want, max_score=bound)
            n_over = int((st == PAIR_OVER_MAX).sum())
            assert n_over == (0 if bound in (0, top) else int((want.score > bound).sum()))
            if bound == top - 1:
                assert n_over >= 1


def test_shared_and_unordered_sequences():
    import wfa_amd
    rng = np.random.default_rng(17)
    q = _rand(rng, 400)
    targets = [_mutate(rng, q, 0.04 + 0.002 * j) for j in range(50)]
    packed, offs = _lay([q] + targets)  # the query packed ONCE
    q_len = np.full(50, len(q), np.uint32)
    t_len = np.array([len(t) for t in targets], np.uint32)
    arrays = wfa_amd.make_blob([q] * 50, targets)
    rev = wfa_amd.make_blob([q] * 50, targets[::-1])
    # a target that serves as the query of another pair
    chain = wfa_amd.make_blob([q, targets[0], targets[1]], [targets[0], targets[1], q])
    chain_pk = (packed, offs[[0, 1, 2]], chain[2], offs[[1, 2, 0]], chain[4])
    for glob, adaptive in MODES:
        al = _aligner(glob, adaptive)
        st, sc, _ = _three(al, arrays, (packed, np.full(50, offs[0], np.uint64), q_len, offs[1:], t_len), _oracle(arrays, glob, adaptive))
        st_r, sc_r, _ = _three(al, rev, (packed, np.full(50, offs[0], np.uint64), q_len, offs[1:][::-1].copy(), t_len[::-1].copy()),
                               _oracle(rev, glob, adaptive))
        assert np.array_equal(st_r, st[::-1]) and np.array_equal(sc_r, sc[::-1])
        _three(al, chain, chain_pk, _oracle(chain, glob, adaptive))


def test_nothing_beyond_the_sequence_is_read():
    import wfa_amd
    rng = np.random.default_rng(18)
    blob, q_off, q_len, t_off, t_len = wfa_amd.generate_pairs(seed=23, n_pairs=64, length=300, error_rate=0.05)
    qs = [bytes(blob[int(o):int(o) + int(n)]) for o, n in zip(q_off, q_len)]
    ts = [bytes(blob[int(o):int(o) + int(n)]) for o, n in zip(t_off, t_len)]
    for ln in (2100, 2101, 3000, 2049):  # for the long kernel (gate at one pair) in global mode, the gather in semi-global mode
        p = _pair_of(rng, ln, 0.02)
        qs.append(p[0]), ts.append(p[1])
    assert any(len(s) % 16 for s in qs + ts)
    arrays = wfa_amd.make_blob(qs, ts)
    clean = _pack(arrays)
    n = len(qs)
    # the same batch re-laid with gaps between the sequences; every gap word, every pad word and every bit beyond a sequence's last
    # base is garbage: random, so a query's differs from its target's, and all ones in every fourth sequence
    dirty, offs = _lay(qs + ts, gap=3)
    junk = rng.integers(0, 1 << 32, size=len(dirty), dtype=np.uint64).astype(np.uint32)
    is_data = np.zeros(len(dirty), bool)
    for j, (s, o) in enumerate(zip(qs + ts, offs)):
        nw, tail = (len(s) + 15) // 16, len(s) % 16
        if j % 4 == 0:
            junk[int(o):int(o) + nw + 4] = 0xFFFFFFFF
        is_data[int(o):int(o) + nw] = True
        if tail:
            keep = np.uint32((1 << (2 * tail)) - 1)
            dirty[int(o) + nw - 1] = (dirty[int(o) + nw - 1] & keep) | (junk[int(o) + nw - 1] & ~keep)
    dirty = np.where(is_data, dirty, junk)
    assert not np.array_equal(dirty[:len(clean[0])], clean[0])
    dirty_pk = (dirty, offs[:n].copy(), arrays[2], offs[n:].copy(), arrays[4])
    for pen, modes in (((4, 6, 2), MODES), ((5, 7, 3), [(True, ADAPT), (False, ADAPT)])):
        for glob, adaptive in modes:
            want = _oracle(arrays, glob, adaptive, pen)
            al = _aligner(glob, adaptive, pen, long_min=1)
            st_c, sc_c, tc = _three(al, arrays, clean, want)
            st_d, sc_d, td = _three(al, arrays, dirty_pk, want)
            assert np.array_equal(st_c, st_d) and np.array_equal(sc_c, sc_d)
            assert (tc.main_kernel_kind, tc.n_retried_pairs) == (td.main_kernel_kind, td.n_retried_pairs)
            if pen == (5, 7, 3):
                assert td.n_retried_pairs == n  # the gather clears the tails for the full path
            elif not glob:
                assert 4 <= td.n_retried_pairs < n  # the long reads: gathered
            elif adaptive is not None:
                assert td.n_retried_pairs == 0  # the long reads: wfa_score_long_kernel, on the caller's words


def test_chaining_score_then_align_on_one_buffer():
    import wfa_amd
    arrays = wfa_amd.generate_pairs(seed=24, n_pairs=2000, length=300, error_rate=0.08)
    packed, qw, q_len, tw, t_len = _pack(arrays)
    keep = packed.copy()
    want = _oracle(arrays, True, ADAPT)
    bound = int(np.median(want.score))
    al = _aligner(True, ADAPT)
    st, sc, _ = _three(al, arrays, (packed, qw, q_len, tw, t_len), want, max_score=bound)
    ok = st == 0
    assert ok.any() and (~ok).any()
    got = al.align_arrays_packed(packed, qw[ok], q_len[ok], tw[ok], t_len[ok])  # a subset of the same offsets, the same words
    assert (got.status == 0).all() and np.array_equal(got.score, sc[ok]) and np.array_equal(got.score, want.score[ok])
    assert np.array_equal(packed, keep)
