"""GPU: the reverse-strand score entries (wfahip_score_batch_packed_rc, wfahip_score_matrix_rc).  Every comparison has three sides:
the new entry on the caller's words with flags; the oracle on bytes reverse-complemented on the host; and the EXISTING packed entry
on a buffer whose flagged queries were reverse-complemented and packed on the host -- against which the routing (main_kernel_kind,
n_retried_pairs) must be equal too: the same pairs on the same kernels."""
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
ADAPT = (10, 50, 1)
MODES = [(True, ADAPT), (True, None), (False, ADAPT), (False, None)]  # (global alignment, wf-adaptive)
MAX_SEQ_LEN = (1 << 29) - 1
PAIR_EMPTY, PAIR_TOO_LONG, PAIR_OVER_MAX = 1, 2, 8
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")  # every other byte is its own complement


def _revcomp(s):
    return s.translate(COMP)[::-1]


def _aligner(glob=True, adaptive=ADAPT, pen=(4, 6, 2), long_min=None):
    import wfa_amd
    al = wfa_amd.New(wfa_amd.Penalties(*pen), wfa_amd.Options(GlobalAlignment=glob), device=0)
    if adaptive is not None:
        assert al.AdaptiveReduction(wfa_amd.AdaptiveReductionOption(*adaptive)) is None
    if long_min is not None:
        al.set_option("score_long_min", long_min)
    return al


def _oracle(qs, ts, glob, adaptive, pen=(4, 6, 2)):
    import wfa_amd
    return O.align_batch(O.make_params(*pen, global_alignment=glob, adaptive=adaptive), *wfa_amd.make_blob(qs, ts), n_threads=16, want_ops=False)


def _expected(want, max_score=0):
    st = want.status.astype(np.int32).copy()
    if max_score:
        st[(want.status == 0) & (want.score > max_score)] = PAIR_OVER_MAX
    return st, np.where(st == 0, want.score, 0).astype(np.uint32)


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


def _pack_seq(s, fill=0):
    """one sequence as wfahip_pack_pairs writes it (16 bases per word, code (ascii >> 1) & 3, then the pad word) -- with the bits beyond
    the last base and the pad word holding `fill`"""
    a = np.frombuffer(s, dtype=np.uint8)
    nw = (len(a) + 15) // 16
    codes = np.zeros(nw * 16, dtype=np.uint64)
    codes[:len(a)] = (a >> 1) & 3
    words = (codes.reshape(nw, 16) << (2 * np.arange(16, dtype=np.uint64))).sum(axis=1).astype(np.uint32)
    if fill and len(a) % 16:
        words[-1] |= np.uint32((fill << (2 * (len(a) % 16))) & 0xFFFFFFFF)
    return np.concatenate([words, np.full(1, fill, np.uint32)])


def _lay(seqs, gap=0, fill=0):
    """the sequences packed one after another, `gap` words between them, gaps, pad words and tail bits = fill: (packed, word offsets)"""
    parts, offs, pos = [], [], 0
    for s in seqs:
        w = _pack_seq(s, fill)
        offs.append(pos), parts.append(w), parts.append(np.full(gap, fill, np.uint32))
        pos += len(w) + gap
    return np.concatenate(parts + [np.full(1, fill, np.uint32)]), np.array(offs, dtype=np.uint64)


def _stored(logical, flags):
    """what the caller's buffer holds so that pair i, under its flag, scores logical[i]: the query itself, or its reverse complement"""
    return [_revcomp(q) if f else q for q, f in zip(logical, flags)]


def _three_pk(al, new_pk, flags, host_pk, want, max_score=0):
    """the new entry over new_pk with flags; the existing entry over host_pk (flagged queries reverse-complemented on the host); the oracle"""
    st, sc = al.score_arrays_packed_rc(*new_pk, flags, max_score=max_score)
    tn = al.last_timing()
    st_h, sc_h = al.score_arrays_packed(*host_pk, max_score=max_score)
    th = al.last_timing()
    st_o, sc_o = _expected(want, max_score)
    print("rc: kind", tn.main_kernel_kind, "retried", tn.n_retried_pairs, "| host-materialised: kind", th.main_kernel_kind, "retried", th.n_retried_pairs)
    assert np.array_equal(st, st_o) and np.array_equal(sc, sc_o)
    assert np.array_equal(st, st_h) and np.array_equal(sc, sc_h)
    assert tn.main_kernel_kind == th.main_kernel_kind
    assert tn.n_retried_pairs == th.n_retried_pairs
    return st, sc, tn


def _three(al, logical, ts, flags, want, max_score=0, gap=0, fill=0):
    """pairs (logical[i], ts[i]): the caller's buffer holds the reverse complement of a flagged pair's query"""
    n = len(ts)
    flags = np.asarray(flags, np.uint8)
    q_len = np.array([len(q) for q in logical], np.uint32)
    t_len = np.array([len(t) for t in ts], np.uint32)
    packed, offs = _lay(_stored(logical, flags) + ts, gap, fill)
    host, hoffs = _lay(list(logical) + ts)
    return _three_pk(al, (packed, offs[:n].copy(), q_len, offs[n:].copy(), t_len), flags, (host, hoffs[:n].copy(), q_len, hoffs[n:].copy(), t_len),
                     want, max_score)


def test_word_boundaries():
    rng = np.random.default_rng(41)
    qs, ts = [], []
    for ln in (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257):
        q = _rand(rng, ln)
        sub = bytearray(q)
        for _ in range(min(3, ln)):
            sub[rng.integers(ln)] = b"ACGT"[rng.integers(4)]
        qs.append(q), ts.append(bytes(sub))  # the same length, flag 0
        qs.append(q), ts.append(bytes(sub))  # ... and flag 1
        qs.append(q), ts.append(_mutate(rng, q, 0.06) or b"A")
        qs.append(_mutate(rng, q, 0.06) or b"C"), ts.append(q)
    for n, m in ((1, 40), (17, 300), (300, 16), (16, 33), (257, 64), (33, 1), (40, 1), (64, 257)):
        long_ = _rand(rng, max(n, m))
        start = int(rng.integers(0, max(n, m) - min(n, m) + 1))
        short = _mutate(rng, long_[start:start + min(n, m)], 0.05)[:min(n, m)]
        short = short + _rand(rng, min(n, m) - len(short))
        qs.append(long_ if n >= m else short), ts.append(short if n >= m else long_)
    flags = ((np.arange(len(qs)) + 1) % 2).astype(np.uint8)  # alternate; the query at word offset 0 of the buffer is a flagged one
    for glob, adaptive in MODES:
        want = _oracle(qs, ts, glob, adaptive)
        al = _aligner(glob, adaptive)
        a = _three(al, qs, ts, flags, want, fill=0)
        b = _three(al, qs, ts, flags, want, fill=0xFFFFFFFF)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert (a[2].main_kernel_kind, a[2].n_retried_pairs) == (b[2].main_kernel_kind, b[2].n_retried_pairs)


def test_length_seams():
    rng = np.random.default_rng(42)
    pairs = [_pair_of(rng, ln, 0.02) for ln in list(range(224, 241)) + list(range(2040, 2048)) + list(range(2048, 2061))]
    n_long = 13
    # every pair twice, forward and flagged (the buffer then holds the query's reverse complement)
    qs = [p[0] for p in pairs] * 2
    ts = [p[1] for p in pairs] * 2
    flags = np.repeat(np.array([0, 1], np.uint8), len(pairs))
    for glob in (True, False):
        want = _oracle(qs, ts, glob, ADAPT)
        # long_min 1: the long global pairs run on wfa_score_long_kernel, the flagged ones on the words wfa_rc_words_kernel wrote
        _, _, t = _three(_aligner(glob, ADAPT, long_min=1), qs, ts, flags, want, fill=0xFFFFFFFF)
        if glob:
            assert t.main_kernel_kind == 19 and t.n_retried_pairs == 0  # (2 % under wf-adaptive: no band near 248 diagonals)
        else:
            assert t.main_kernel_kind == 20 and t.n_retried_pairs >= 2 * n_long  # semi-global reads over 2 047 bases: gathered on the host
        # the default gate (64) on fewer long pairs: handed back, gathered with rc_word on the host
        _, _, t = _three(_aligner(glob, ADAPT), qs, ts, flags, want, fill=0xFFFFFFFF)
        assert t.n_retried_pairs >= 2 * n_long
    # only long pairs, all flagged: the short launch is skipped
    lq, lt = [p[0] for p in pairs[-n_long:]], [p[1] for p in pairs[-n_long:]]
    _, _, t = _three(_aligner(True, None, long_min=1), lq, lt, np.ones(n_long, np.uint8), _oracle(lq, lt, True, None))
    assert t.main_kernel_kind == 23


@pytest.mark.parametrize("pen", [(4, 6, 2), (5, 7, 3)])
def test_penalty_routes(pen):
    import wfa_amd
    blob, q_off, q_len, t_off, t_len = wfa_amd.generate_pairs(seed=43, n_pairs=256, length=300, error_rate=0.05)
    qs = [bytes(blob[int(o):int(o) + int(n)]) for o, n in zip(q_off, q_len)]
    ts = [bytes(blob[int(o):int(o) + int(n)]) for o, n in zip(t_off, t_len)]
    flags = (np.random.default_rng(43).random(256) < 0.5).astype(np.uint8)
    for glob in (True, False):
        _, _, t = _three(_aligner(glob, ADAPT, pen), qs, ts, flags, _oracle(qs, ts, glob, ADAPT, pen))
        if pen == (5, 7, 3):  # no instance: every pair is handed back and gathered
            assert t.n_retried_pairs == 256
        else:
            assert t.main_kernel_kind == (19 if glob else 20) and t.n_retried_pairs <= 10


def test_band_the_ring_cannot_hold():
    import wfa_amd
    rng = np.random.default_rng(44)
    blob, q_off, q_len, t_off, t_len = wfa_amd.generate_pairs(seed=44, n_pairs=100, length=300, error_rate=0.05)
    qs = [bytes(blob[int(o):int(o) + int(n)]) for o, n in zip(q_off, q_len)]
    ts = [bytes(blob[int(o):int(o) + int(n)]) for o, n in zip(t_off, t_len)]
    wide = (3, 50, 77, 103)
    for at in wide:  # two unrelated reads: the band outgrows the ring's 248 diagonals long before they end
        qs.insert(at, _rand(rng, 600)), ts.insert(at, _rand(rng, 600))
    flags = (np.arange(len(qs)) % 3 == 0).astype(np.uint8)
    flags[list(wide)] = 1  # the pairs of the fallback are flagged
    _, _, t = _three(_aligner(True, None), qs, ts, flags, _oracle(qs, ts, True, None), fill=0xFFFFFFFF)
    assert t.main_kernel_kind == 19 and t.n_retried_pairs >= 4


@pytest.mark.parametrize("pen", [(4, 6, 2), (5, 7, 3)])
@pytest.mark.parametrize("glob", [True, False])
def test_statuses_and_the_bound(glob, pen):
    rng = np.random.default_rng(45)
    qs = [_rand(rng, int(rng.integers(100, 400))) for _ in range(24)]
    ts = [_mutate(rng, q, float(rng.uniform(0.02, 0.15))) for q in qs]
    qs[2], ts[5] = b"", b""  # an empty query, an empty target
    flags = (np.arange(24) % 2).astype(np.uint8)
    flags[[2, 5, 6]] = 1  # the empty and the too long pairs carry set flags
    n = 24
    packed, offs = _lay(_stored(qs, flags) + ts)
    host, hoffs = _lay(qs + ts)
    q_len = np.array([len(q) for q in qs], np.uint32)
    t_len = np.array([len(t) for t in ts], np.uint32)
    q_len[6] = MAX_SEQ_LEN + 1  # too long: its offsets are never looked at
    qw, tw, hqw, htw = offs[:n].copy(), offs[n:].copy(), hoffs[:n].copy(), hoffs[n:].copy()
    for a in (qw, hqw):
        a[6], a[2] = np.uint64(1 << 40), np.uint64((1 << 64) - 1)
    for a in (tw, htw):
        a[2], a[5] = np.uint64(1 << 41), np.uint64(1 << 63)
    res = _oracle(qs, ts, glob, ADAPT, pen)
    want = SimpleNamespace(status=np.array(res.status), score=np.array(res.score))  # the oracle's answer, the pair made too long put right
    want.status[6], want.score[6] = PAIR_TOO_LONG, 0
    ok = want.status == 0
    al = _aligner(glob, ADAPT, pen)
    top = int(want.score[ok].max())
    for bound in (0, int(np.median(want.score[ok])), top, top - 1):
        st, _, t = _three_pk(al, (packed, qw, q_len, tw, t_len), flags, (host, hqw, q_len, htw, t_len), want, max_score=bound)
        assert st[2] == PAIR_EMPTY and st[5] == PAIR_EMPTY and st[6] == PAIR_TOO_LONG
        n_over = int((st == PAIR_OVER_MAX).sum())
        assert n_over == (0 if bound in (0, top) else int((want.score[ok] > bound).sum()))
        if bound not in (0, top, top - 1):  # (the median: pairs of both strands are over it)
            assert ((st == PAIR_OVER_MAX) & (flags == 1)).any() and ((st == PAIR_OVER_MAX) & (flags == 0)).any()
        if pen == (5, 7, 3):
            assert t.n_retried_pairs == n


def test_both_strands_by_repetition():
    rng = np.random.default_rng(46)
    ts = [_rand(rng, int(rng.integers(150, 500))) for _ in range(40)]
    # the buffer's queries: the reverse complement of a mutated target; two palindromes (their own reverse complement)
    qs = [_revcomp(_mutate(rng, t, 0.04)) for t in ts]
    for i, k in ((7, 40), (23, 75)):
        qs[i] = b"ACGT" * k
        ts[i] = _mutate(rng, qs[i], 0.04)
        assert _revcomp(qs[i]) == qs[i]
    n = len(qs)
    packed, offs = _lay(qs + ts, gap=1, fill=0xFFFFFFFF)  # every sequence ONCE
    q_len = np.array([len(q) for q in qs], np.uint32)
    t_len = np.array([len(t) for t in ts], np.uint32)
    twice = lambda a: np.concatenate([a, a])
    flags = np.repeat(np.array([0, 1], np.uint8), n)
    new_pk = (packed, twice(offs[:n]), twice(q_len), twice(offs[n:]), twice(t_len))
    logical = qs + [_revcomp(q) for q in qs]
    host, hoffs = _lay(logical + ts)
    host_pk = (host, hoffs[:2 * n].copy(), twice(q_len), twice(hoffs[2 * n:]), twice(t_len))
    for glob, adaptive in MODES:
        al = _aligner(glob, adaptive)
        st, sc, _ = _three_pk(al, new_pk, flags, host_pk, _oracle(logical, ts + ts, glob, adaptive))
        st_e, sc_e = al.score_arrays_packed(packed, offs[:n].copy(), q_len, offs[n:].copy(), t_len)  # the flag-0 half: the existing entry's output
        assert np.array_equal(st[:n], st_e) and np.array_equal(sc[:n], sc_e)
        assert (st == 0).all()
        rest = np.ones(n, bool)
        rest[[7, 23]] = False
        assert (sc[n:][rest] < sc[:n][rest]).all()  # the reverse strand is the low one
        assert sc[7] == sc[n + 7] and sc[23] == sc[n + 23]  # a palindromic query scores the same on both strands


def _matrix_want(qs, ts, flags, glob, adaptive, pen=(4, 6, 2)):
    eq = [_revcomp(q) if f else q for q, f in zip(qs, flags)]
    want = _oracle([q for q in eq for _ in ts], [t for _ in eq for t in ts], glob, adaptive, pen)
    st, sc = _expected(want)
    return st.reshape(len(qs), len(ts)), sc.reshape(len(qs), len(ts))


@pytest.mark.parametrize("glob,adaptive", MODES)
def test_matrix(glob, adaptive):
    import wfa_amd
    rng = np.random.default_rng(47)
    anc = _rand(rng, 330)
    ts = [_mutate(rng, anc[:ln], 0.05) for ln in (330, 257, 64, 300, 31, 200, 330)]
    qs = [_mutate(rng, anc, 0.05), _revcomp(_mutate(rng, anc[:256], 0.05)), _revcomp(_mutate(rng, anc, 0.04)), _mutate(rng, anc[:17], 0.0),
          _revcomp(_mutate(rng, anc[:120], 0.05)[:60] + b"N" + _mutate(rng, anc[60:120], 0.05) + b"acgt")]
    flags = np.array([0, 1, 1, 0, 1], np.uint8)
    wst, wsc = _matrix_want(qs, ts, flags, glob, adaptive)
    blob, off, ln, _, _ = wfa_amd.make_blob(qs + ts, [b""] * 12)
    al = _aligner(glob, adaptive)
    for tile in (3, 14):  # 3: a row in three tiles of columns; 14: two rows per tile, the last tile one row
        al.set_option("matrix_tile_cells", tile)
        status, score = np.full((5, 10), -7, np.int32), np.full((5, 10), 7, np.uint32)
        st, sc = al.score_matrix_arrays(blob, off[:5], ln[:5], off[5:], ln[5:], out=(status[:, 2:9], score[:, 2:9]), q_rc=flags)
        t = al.last_timing()
        assert np.array_equal(st, wst) and np.array_equal(sc, wsc)
        assert (status[:, :2] == -7).all() and (status[:, 9:] == -7).all() and (score[:, :2] == 7).all() and (score[:, 9:] == 7).all()
        assert t.main_kernel_kind == (21 if glob else 22)
        assert t.n_retried_pairs >= 7  # the row of the query with an N
        if adaptive is not None:
            assert t.n_retried_pairs < 35
    # the rows without a byte outside ACGT: what the packed pair-list entry gives for the same pairs
    al.set_option("matrix_tile_cells", 0)
    packed, offs = _lay(qs[:4] + ts)
    rows = np.repeat(np.arange(4), 7)
    cols = np.tile(np.arange(7), 4)
    st_p, sc_p = al.score_arrays_packed_rc(packed, offs[rows], ln[:4][rows], offs[4 + cols], ln[5:][cols], flags[rows])
    assert np.array_equal(st_p.reshape(4, 7), wst[:4]) and np.array_equal(sc_p.reshape(4, 7), wsc[:4])
    # ScoreMatrix(strands="both"): the per-cell best of two explicit calls
    st_b, sc_b, strand = al.ScoreMatrix(qs, ts, strands="both")
    f = al.score_matrix_arrays(blob, off[:5], ln[:5], off[5:], ln[5:])
    r = al.score_matrix_arrays(blob, off[:5], ln[:5], off[5:], ln[5:], q_rc=np.ones(5, np.uint8))
    e_st, e_sc, e_strand = wfa_amd.best_strand(f[0], f[1], r[0], r[1])
    assert np.array_equal(st_b, e_st) and np.array_equal(sc_b, e_sc) and np.array_equal(strand, e_strand)
    assert strand[1, 0] == 1 and strand[2, 0] == 1 and strand[0, 0] == 0
    # ... and all against all (ts=None): each query in both orientations against every query as it stands
    st_a, sc_a, strand_a = al.ScoreMatrix(qs, strands="both")
    f = al.score_matrix_arrays(blob, off[:5], ln[:5], off[:5], ln[:5])
    r = al.score_matrix_arrays(blob, off[:5], ln[:5], off[:5], ln[:5], q_rc=np.ones(5, np.uint8))
    e_st, e_sc, e_strand = wfa_amd.best_strand(f[0], f[1], r[0], r[1])
    assert np.array_equal(st_a, e_st) and np.array_equal(sc_a, e_sc) and np.array_equal(strand_a, e_strand)
    assert strand_a[0, 1] == 1 and strand_a[1, 0] == 1 and not strand_a.diagonal()[:4].any()  # (a sequence against itself: forward, score 0)


@pytest.mark.parametrize("glob", [True, False])
def test_matrix_over_the_same_arrays(glob):
    """queries and targets are the same arrays: the table holds a sequence once, reverse-complemented in a flagged row and forward in
    its column -- among them two reads beyond 2 047 bases (global: wfa_score_long_kernel<MATRIX> on the words of wfa_rc_words_kernel)"""
    import wfa_amd
    rng = np.random.default_rng(48)
    anc, lanc = _rand(rng, 300), _rand(rng, 2200)
    seqs = [_mutate(rng, anc, 0.05), _revcomp(_mutate(rng, anc, 0.05)), _mutate(rng, anc[:130], 0.05), _revcomp(_mutate(rng, anc[:257], 0.05)),
            _mutate(rng, lanc, 0.02), _revcomp(_mutate(rng, lanc[:2100], 0.02))]
    flags = np.array([0, 1, 0, 1, 0, 1], np.uint8)
    wst, wsc = _matrix_want(seqs, seqs, flags, glob, ADAPT)
    blob, off, ln, _, _ = wfa_amd.make_blob(seqs, [b""] * 6)
    al = _aligner(glob, ADAPT, long_min=1)
    al.set_option("matrix_tile_cells", 8)
    st, sc = al.score_matrix_arrays(blob, off, ln, off, ln, q_rc=flags)
    t = al.last_timing()
    print("same arrays: kind", t.main_kernel_kind, "retried", t.n_retried_pairs)
    assert np.array_equal(st, wst) and np.array_equal(sc, wsc)
    if glob:
        # the flagged rows found their forward relatives: a hundred bases of gap and 4 % of edits on 2 100 bases, 10 % of edits on 300
        assert sc[5, 4] < 2200 and sc[1, 0] < 400
        assert t.n_retried_pairs < 36 - 4  # (the related long cells ran on the long kernel)


@pytest.mark.parametrize("long_rows", [(), (0,), (5,), (0, 5)])
def test_matrix_flagged_short_rows_against_long_columns(long_rows):
    """global, the gate at one cell: wfa_score_long_kernel<MATRIX> takes every cell with a long side, so a flagged query of 2 000 bases
    against a related target of 2 100 is read from the words wfa_rc_words_kernel wrote -- alone, and with a flagged long row before it,
    behind it and on both sides of it in the table"""
    import wfa_amd
    rng = np.random.default_rng(49)
    anc = _rand(rng, 2150)
    ts = [_mutate(rng, anc[:ln], 0.02) for ln in (2100, 2120, 2090, 1990)]
    qs = [_revcomp(_mutate(rng, anc[:2000], 0.02)), _mutate(rng, anc[:2010], 0.02), _revcomp(_mutate(rng, anc[:1985], 0.02)),
          _revcomp(_mutate(rng, anc[:2047], 0.02))]
    flags = [1, 0, 1, 1]
    for at in sorted(long_rows):  # a flagged long row, at the front and / or at the end of the table's rows
        qs.insert(min(at, len(qs)), _revcomp(_mutate(rng, anc[:2140], 0.02))), flags.insert(min(at, len(flags)), 1)
    flags = np.array(flags, np.uint8)
    wst, wsc = _matrix_want(qs, ts, flags, True, ADAPT)
    assert (wst == 0).all() and wsc.max() < 1500  # related in the orientation the flags name
    blob, off, ln, _, _ = wfa_amd.make_blob(qs + ts, [b""] * (len(qs) + 4))
    n = len(qs)
    al = _aligner(True, ADAPT, long_min=1)
    for tile in (0, 3):
        al.set_option("matrix_tile_cells", tile)
        st, sc = al.score_matrix_arrays(blob, off[:n], ln[:n], off[n:], ln[n:], q_rc=flags)
        t = al.last_timing()
        print("short rows, long columns: kind", t.main_kernel_kind, "retried", t.n_retried_pairs)
        assert np.array_equal(st, wst) and np.array_equal(sc, wsc)
        assert t.n_retried_pairs == 0  # (2 % under wf-adaptive: no band near 248 diagonals; the kernels, not the full path, scored them)


def test_one_flagged_long_query_against_many_targets():
    """the pair list: one flagged long query listed against five long targets, and the same offset with a shorter length -- the
    reverse complement of a prefix is not a prefix of the reverse complement"""
    rng = np.random.default_rng(50)
    full = _rand(rng, 2100)  # what the flagged pairs score: the reverse complement of the stored query
    stored = _revcomp(full)
    ts = [_mutate(rng, full, 0.02) for _ in range(5)] + [_mutate(rng, _revcomp(stored[:2060]), 0.02), _mutate(rng, stored, 0.02)]
    logical = [full] * 5 + [_revcomp(stored[:2060]), stored]
    flags = np.array([1, 1, 1, 1, 1, 1, 0], np.uint8)
    q_len = np.array([len(q) for q in logical], np.uint32)
    t_len = np.array([len(t) for t in ts], np.uint32)
    packed, offs = _lay([stored] + ts, gap=2, fill=0xFFFFFFFF)  # the query ONCE
    host, hoffs = _lay(logical + ts)
    al = _aligner(True, ADAPT, long_min=1)
    _, sc, t = _three_pk(al, (packed, np.full(7, offs[0], np.uint64), q_len, offs[1:].copy(), t_len), flags,
                         (host, hoffs[:7].copy(), q_len, hoffs[7:].copy(), t_len), _oracle(logical, ts, True, ADAPT))
    assert t.main_kernel_kind == 23 and t.n_retried_pairs == 0 and sc.max() < 1000
