"""GPU: the screen on device-resident 2-bit words (wfahip_score_batch_packed_device; Aligner.score_tensors_packed) and its survivors
(wfahip_select_pairs_device; Aligner.select_tensors).  One helper compares three things: the device entry's status and score with
score_arrays_packed_rc on the SAME words, offsets, lengths and flags; (main_kernel_kind, n_retried_pairs, arena_bytes == 0) with that
host entry's; and, without a bound, status and score with the oracle on the bytes (revcomp(q) if flagged else q, t).  After every call
of the new entry its input tensors must hold what they held before."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from oracle import oracle as O
from test_score_rc_gpu import ADAPT, MAX_SEQ_LEN, MODES, _lay, _mutate, _pair_of, _rand, _revcomp, _stored

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PAIR_EMPTY, PAIR_TOO_LONG, PAIR_OVER_MAX = 1, 2, 8
SLACK = 4       # words behind the caller's words, which the entry may read
SD_TILE = 1024  # items per tile of the router's selections (wfa_amd/csrc/wfa_score_dev.hpp)


def _aligner(glob=True, adaptive=ADAPT, pen=(4, 6, 2), opts=None):
    import wfa_amd
    al = wfa_amd.New(wfa_amd.Penalties(*pen), wfa_amd.Options(GlobalAlignment=glob), device=0)
    if adaptive is not None:
        assert al.AdaptiveReduction(wfa_amd.AdaptiveReductionOption(*adaptive)) is None
    for k, v in (opts or {}).items():
        al.set_option(k, v)
    return al


def _oracle(qs, ts, glob, adaptive, pen=(4, 6, 2)):
    import wfa_amd
    w = O.align_batch(O.make_params(*pen, global_alignment=glob, adaptive=adaptive), *wfa_amd.make_blob(qs, ts), n_threads=16, want_ops=False)
    return w.status.astype(np.int32), np.where(w.status == 0, w.score, 0).astype(np.uint32)


def _dev(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to("cuda:0")


def _to_device(pk, flags):
    """the caller's arrays as the tensors score_tensors_packed takes, four words of slack (ones) behind the words; flags None = no tensor"""
    packed, q_woff, q_len, t_woff, t_len = pk
    words = np.concatenate([np.asarray(packed, np.uint32), np.full(SLACK, 0xFFFFFFFF, np.uint32)])
    return [_dev(words, np.int32), _dev(np.asarray(q_woff, np.uint64), np.int64), _dev(np.asarray(q_len, np.uint32), np.int32),
            _dev(np.asarray(t_woff, np.uint64), np.int64), _dev(np.asarray(t_len, np.uint32), np.int32),
            None if flags is None else _dev(np.asarray(flags, np.uint8), np.uint8)]


def _tm(al):
    t = al.last_timing()
    return t.main_kernel_kind, t.n_retried_pairs, t.arena_bytes == 0


def _call(al, tens, max_score=0, out=None, stream=None):
    before = [t.clone() if t is not None else None for t in tens]
    st, sc = al.score_tensors_packed(*tens[:5], q_rc=tens[5], max_score=max_score, out=out, stream=stream)
    tm = _tm(al)
    for a, b in zip(tens, before):
        assert a is None or bool((a == b).all()), "an input tensor was written"
    n = tens[2].numel()
    return st.cpu().numpy()[:n], sc.cpu().numpy().view(np.uint32)[:n], tm


def _check(al, pk, flags, want=None, max_score=0, what=""):
    """the device entry over pk and flags against the host entry on the same arrays, and -- want = the oracle's (status, score), without a
    bound -- against the oracle.  Returns the device entry's (status, score, (kind, retried, arena_bytes == 0))"""
    st, sc, tn = _call(al, _to_device(pk, flags), max_score)
    hst, hsc = al.score_arrays_packed_rc(*pk, flags, max_score=max_score)
    th = _tm(al)
    print(what, "| device (kind, retried, no arena)", tn, "| host entry", th, "| mismatches: status", int((st != hst).sum()), "score", int((sc != hsc).sum()))
    assert np.array_equal(st, hst) and np.array_equal(sc, hsc), what
    assert tn == th, what
    if want is not None and max_score == 0:
        assert np.array_equal(st, want[0]) and np.array_equal(sc, want[1]), what + ": against the oracle"
    return st, sc, tn


def _buffers(logical, ts, flags, gap=0, fill=0):
    """pairs (logical[i], ts[i]): the caller's buffer holds the reverse complement of a flagged pair's query"""
    n = len(ts)
    packed, offs = _lay(_stored(logical, flags) + list(ts), gap, fill)
    return (packed, offs[:n].copy(), np.array([len(q) for q in logical], np.uint32), offs[n:].copy(), np.array([len(t) for t in ts], np.uint32))


def _generated(seed, n, length, rate):
    import wfa_amd
    blob, q_off, q_len, t_off, t_len = wfa_amd.generate_pairs(seed=seed, n_pairs=n, length=length, error_rate=rate)
    qs = [bytes(blob[int(o):int(o) + int(k)]) for o, k in zip(q_off, q_len)]
    ts = [bytes(blob[int(o):int(o) + int(k)]) for o, k in zip(t_off, t_len)]
    return qs, ts


def _golden_pairs():
    """the golden pairs a packed buffer can hold: pure uppercase ACGT"""
    ka = json.load(open(os.path.join(GOLDEN, "known_answers.json")))["vectors"]
    ref = json.load(open(os.path.join(GOLDEN, "ref_test_pairs.json")))
    pairs = [(v["q"].encode(), v["t"].encode()) for v in ka] + [(p["q"].encode(), p["t"].encode()) for p in ref]
    return [(q, t) for q, t in pairs if re.fullmatch(rb"[ACGT]*", q) and re.fullmatch(rb"[ACGT]*", t)]


_BATCHES = {}


def _batch(name):
    """the batches of case 1, made once: (logical queries, targets, random flags)"""
    if not _BATCHES:
        g = _golden_pairs()
        _BATCHES["golden"] = ([q for q, _ in g], [t for _, t in g])
        _BATCHES["300"] = _generated(101, 512, 300, 0.05)
        _BATCHES["1000"] = _generated(102, 256, 1000, 0.05)
    qs, ts = _BATCHES[name]
    return qs, ts, (np.random.default_rng(103).random(len(qs)) < 0.5).astype(np.uint8)


# ---- 1. golden and generated pairs
@pytest.mark.parametrize("glob,adaptive", MODES)
@pytest.mark.parametrize("name", ["golden", "300", "1000"])
def test_golden_and_generated(name, glob, adaptive):
    qs, ts, flags = _batch(name)
    assert len(qs) > 8
    want = _oracle(qs, ts, glob, adaptive)
    al = _aligner(glob, adaptive)
    try:
        _check(al, _buffers(qs, ts, flags, fill=0xFFFFFFFF), flags, want, what=f"{name}, random flags")
        zeros = np.zeros(len(qs), np.uint8)
        pk = _buffers(qs, ts, zeros)
        _, _, tz = _check(al, pk, zeros, want, what=f"{name}, zero flags")
        _, _, tn = _check(al, pk, None, want, what=f"{name}, no flags")
        assert tz == tn
    finally:
        al.close()


# ---- 2. the seams of the router and of the word layout
@pytest.mark.parametrize("glob", [True, False])
@pytest.mark.parametrize("window", [None, 16])
def test_seams(glob, window):
    rng = np.random.default_rng(104)
    pairs = [_pair_of(rng, ln, 0.02) for ln in (1, 15, 16, 17, 31, 32, 33, 2046, 2047, 2048, 2049)]
    qs, ts = [p[0] for p in pairs] * 2, [p[1] for p in pairs] * 2
    flags = np.repeat(np.array([0, 1], np.uint8), len(pairs))
    opts = {"score_long_min": 1}
    if window:
        opts["score_long_window_words"] = window
    al = _aligner(glob, ADAPT, opts=opts)
    try:
        _, _, t = _check(al, _buffers(qs, ts, flags, fill=0xFFFFFFFF), flags, _oracle(qs, ts, glob, ADAPT), what=f"seams, window {window}")
        if glob:
            assert t[0] == 19 and t[1] == 0, t  # (the long pairs on wfa_score_long_kernel, the flagged ones from the scratch words)
        else:
            assert t[0] == 20 and t[1] >= 4, t  # semi-global reads over 2 047 bases: gathered on the device
    finally:
        al.close()


# ---- 3. penalty shapes
@pytest.mark.parametrize("pen", [(4, 6, 2), (2, 4, 2), (1, 1, 1), (4, 4, 2), (6, 4, 2), (5, 7, 3)])
@pytest.mark.parametrize("glob", [True, False])
def test_penalty_shapes(pen, glob):
    qs, ts = _generated(105, 256, 300, 0.05)
    qs, ts = list(qs), list(ts)
    n = len(qs)
    flags = (np.random.default_rng(105).random(n) < 0.5).astype(np.uint8)
    no_instance = pen == (5, 7, 3)
    if no_instance:  # every pair goes through the gather kernel: among them empty and too long ones, flagged and not
        qs[2], ts[5], qs[9] = b"", b"", b""
        flags[[2, 5, 6]] = 1
        flags[9] = 0
    pk = _buffers(qs, ts, flags, gap=1, fill=0xFFFFFFFF)
    wst, wsc = _oracle(qs, ts, glob, ADAPT, pen)
    if no_instance:
        pk[2][6] = MAX_SEQ_LEN + 1  # too long: its offsets are never looked at
        pk[1][6], pk[1][2] = np.uint64(1 << 63), np.uint64((1 << 64) - 1)
        pk[3][5], pk[3][9] = np.uint64(1 << 63), np.uint64(1 << 41)
        wst[6], wsc[6] = PAIR_TOO_LONG, 0
    al = _aligner(glob, ADAPT, pen)
    try:
        st, _, t = _check(al, pk, flags, (wst, wsc), what=f"penalties {pen}")
        if no_instance:
            assert t[1] == n, t
            assert st[2] == PAIR_EMPTY and st[5] == PAIR_EMPTY and st[9] == PAIR_EMPTY and st[6] == PAIR_TOO_LONG
        elif pen == (4, 6, 2):
            assert t[0] == (19 if glob else 20) and t[1] <= 10, t
    finally:
        al.close()


# ---- 4. the pairs the kernels hand back
def test_hand_back_band():
    """a 1 500-base pair at 20 % without wf-adaptive among short pairs: its band outgrows the ring's 248 diagonals"""
    rng = np.random.default_rng(106)
    qs, ts = map(list, _generated(106, 100, 300, 0.05))
    for at, f in ((3, 1), (50, 0)):
        q = _rand(rng, 1500)
        qs.insert(at, q), ts.insert(at, _mutate(rng, q, 0.20))
    flags = (np.arange(len(qs)) % 3 == 0).astype(np.uint8)
    al = _aligner(True, None)
    try:
        _, _, t = _check(al, _buffers(qs, ts, flags, fill=0xFFFFFFFF), flags, _oracle(qs, ts, True, None), what="band")
        assert t[0] == 19 and t[1] >= 2 and not t[2], t
    finally:
        al.close()


def test_hand_back_semi_global_long_target():
    rng = np.random.default_rng(107)
    qs, ts = map(list, _generated(107, 100, 300, 0.05))
    for at, f in ((7, 1), (60, 0)):
        t = _rand(rng, 2300)
        ts.insert(at, t), qs.insert(at, _mutate(rng, t[400:1900], 0.03))
    flags = (np.arange(len(qs)) % 2).astype(np.uint8)
    assert flags[7] == 1 and flags[60] == 0
    al = _aligner(False, ADAPT)
    try:
        _, _, t = _check(al, _buffers(qs, ts, flags, fill=0xFFFFFFFF), flags, _oracle(qs, ts, False, ADAPT), what="semi-global, 2 300-base target")
        assert t[0] == 20 and t[1] >= 2, t
    finally:
        al.close()


_LONG = {}


@pytest.mark.parametrize("n_long", [63, 64])
def test_hand_back_below_the_gate_and_kind_23_at_it(n_long):
    """63 pairs of 3 kbp at the default gate take the full path; 64 run on wfa_score_long_kernel"""
    if not _LONG:
        qs, ts = _generated(108, 64, 3000, 0.02)
        _LONG["p"] = (qs, ts, _oracle(qs, ts, True, ADAPT))
    qs, ts, want = _LONG["p"]
    qs, ts, want = qs[:n_long], ts[:n_long], (want[0][:n_long], want[1][:n_long])
    flags = (np.arange(n_long) % 3 == 1).astype(np.uint8)
    al = _aligner(True, ADAPT)
    try:
        _, _, t = _check(al, _buffers(qs, ts, flags, fill=0xFFFFFFFF), flags, want, what=f"{n_long} long pairs")
        if n_long == 63:
            assert t[0] == 19 and t[1] == 63 and not t[2], t
        else:
            assert t[0] == 23 and t[1] == 0 and t[2], t
    finally:
        al.close()


# ---- 5. one flagged long query against eight long targets
def test_one_flagged_long_query_against_eight_targets():
    """by repeated offsets, the targets listed in reverse order of their offsets; and the same offset under a shorter length: the
    reverse complement of a prefix is not a prefix of the reverse complement"""
    rng = np.random.default_rng(109)
    full = _rand(rng, 2100)  # what the flagged pairs score: the reverse complement of the stored query
    stored = _revcomp(full)
    ts = [_mutate(rng, full, 0.02) for _ in range(8)] + [_mutate(rng, _revcomp(stored[:2060]), 0.02), _mutate(rng, stored, 0.02)]
    logical = [full] * 8 + [_revcomp(stored[:2060]), stored]
    flags = np.array([1] * 9 + [0], np.uint8)
    packed, offs = _lay(ts[::-1] + [stored], gap=2, fill=0xFFFFFFFF)  # the query ONCE, behind the targets
    n = len(ts)
    pk = (packed, np.full(n, offs[n], np.uint64), np.array([len(q) for q in logical], np.uint32), offs[:n][::-1].copy(),
          np.array([len(t) for t in ts], np.uint32))
    al = _aligner(True, ADAPT, opts={"score_long_min": 1})
    try:
        _, sc, t = _check(al, pk, flags, _oracle(logical, ts, True, ADAPT), what="one query, eight targets")
        assert t[0] == 23 and t[1] == 0 and sc.max() < 1000, t
    finally:
        al.close()


# ---- 6. garbage in tail bits, pad words and between the sequences
@pytest.mark.parametrize("glob,adaptive", [(True, None), (False, ADAPT)])
def test_garbage(glob, adaptive):
    rng = np.random.default_rng(110)
    pairs = [_pair_of(rng, int(rng.integers(1, 400)), 0.05) for _ in range(150)]
    pairs += [_pair_of(rng, ln, 0.02) for ln in (2100, 2300, 2049)]  # hand-backs: below the gate / over the wide kernel's length
    q = _rand(rng, 700)
    pairs += [(q, _rand(rng, 700)), (_rand(rng, 650), q)]  # unrelated: a band the global ring cannot hold
    order = rng.permutation(len(pairs))
    qs, ts = [pairs[i][0] for i in order], [pairs[i][1] for i in order]
    flags = (rng.random(len(qs)) < 0.5).astype(np.uint8)
    want = _oracle(qs, ts, glob, adaptive)
    al = _aligner(glob, adaptive)
    try:
        a = _check(al, _buffers(qs, ts, flags), flags, want, what="clean")
        b = _check(al, _buffers(qs, ts, flags, gap=3, fill=0xFFFFFFFF), flags, want, what="garbage")
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
        assert a[2][1] >= 3, a[2]
    finally:
        al.close()


# ---- 7. max_score at the median of a mixed batch
def _mixed(glob):
    """short pairs, long pairs (global: on wfa_score_long_kernel, the gate at 8; semi-global: the wide kernel's four-wave instance) and
    pairs the kernels hand back (global, no wf-adaptive: a band over 248 diagonals; semi-global: a read over 2 047 bases)"""
    rng = np.random.default_rng(111 if glob else 112)
    cls, qs, ts = [], [], []

    def add(c, q, t):
        cls.append(c), qs.append(q), ts.append(t)
    for _ in range(120):
        q = _rand(rng, 400)
        add(0, q, _mutate(rng, q, float(rng.uniform(0.01, 0.35))))
    for _ in range(16):
        q = _rand(rng, 2100 if glob else 1500)
        add(1, q, _mutate(rng, q, float(rng.uniform(0.002, 0.06))))
    for k in range(8):
        if glob:  # one deletion of 140 bases: the band passes 248 diagonals at a score near 290; or 25 % of edits: far over any median
            q = _rand(rng, 600)
            add(2, q, q[:200] + q[340:] if k % 2 == 0 else _mutate(rng, q, 0.25))
        else:
            q = _rand(rng, 2200)
            add(2, q, _mutate(rng, q, 0.004 if k % 2 == 0 else 0.08))
    order = rng.permutation(len(qs))
    return np.array(cls)[order], [qs[i] for i in order], [ts[i] for i in order]


@pytest.mark.parametrize("glob", [True, False])
def test_max_score_at_the_median(glob):
    adaptive = None if glob else ADAPT
    cls, qs, ts = _mixed(glob)
    flags = (np.arange(len(qs)) % 2).astype(np.uint8)
    wst, wsc = _oracle(qs, ts, glob, adaptive)
    assert (wst == 0).all()
    bound = int(np.median(wsc))
    for c in (0, 1, 2):
        assert (wsc[cls == c] > bound).any() and (wsc[cls == c] <= bound).any(), (c, bound, sorted(wsc[cls == c]))
    al = _aligner(glob, adaptive, opts={"score_long_min": 8})
    try:
        pk = _buffers(qs, ts, flags, fill=0xFFFFFFFF)
        st0, sc0, t0 = _check(al, pk, flags, (wst, wsc), what="mixed, no bound")
        assert t0[1] >= 4, t0
        st, sc, _ = _check(al, pk, flags, max_score=bound, what=f"mixed, bound {bound}")
        over = wsc > bound
        assert (st[over] == PAIR_OVER_MAX).all() and not sc[over].any()
        assert np.array_equal(st[~over], st0[~over]) and np.array_equal(sc[~over], sc0[~over])
    finally:
        al.close()


# ---- 8. empty and too long pairs: their offsets are never looked at
@pytest.mark.parametrize("glob", [True, False])
def test_empty_and_too_long_pairs(glob):
    rng = np.random.default_rng(113)
    qs = [_rand(rng, int(rng.integers(100, 400))) for _ in range(24)]
    ts = [_mutate(rng, q, 0.05) for q in qs]
    qs[2], ts[5] = b"", b""
    flags = (np.arange(24) % 2).astype(np.uint8)
    flags[[2, 5, 6]] = 1
    pk = _buffers(qs, ts, flags, fill=0xFFFFFFFF)
    pk[2][6] = MAX_SEQ_LEN + 1
    pk[1][6], pk[1][2], pk[1][5] = np.uint64(1 << 63), np.uint64(1 << 63), np.uint64((1 << 64) - 1)
    pk[3][2], pk[3][5], pk[3][6] = np.uint64(1 << 63), np.uint64(1 << 63), np.uint64(1 << 63)
    qs_o = list(qs)
    qs_o[6] = b""
    wst, wsc = _oracle(qs_o, ts, glob, ADAPT)
    wst[6] = PAIR_TOO_LONG
    al = _aligner(glob, ADAPT)
    try:
        st, _, _ = _check(al, pk, flags, (wst, wsc), what="empty and too long")
        assert st[2] == PAIR_EMPTY and st[5] == PAIR_EMPTY and st[6] == PAIR_TOO_LONG
    finally:
        al.close()


# ---- 9. bounds: the verdict comes before any kernel reads a word
def test_words_that_end_beyond_n_words():
    """packed[:k] of a whole allocation, the last target's pad word at k: nothing is read out of bounds, the call is refused with the
    outputs untouched, and the next call on the context is correct"""
    import torch
    import wfa_amd
    from wfa_amd import _lib
    qs, ts = _generated(114, 200, 300, 0.05)
    flags = (np.arange(len(qs)) % 2).astype(np.uint8)
    pk = _buffers(qs, ts, flags)
    want = _oracle(qs, ts, True, ADAPT)
    tens = _to_device(pk, flags)
    n = len(qs)
    k = int(pk[3][-1]) + (int(pk[4][-1]) + 15) // 16  # the last target's words fit below k, its pad word does not
    assert k == len(pk[0]) - 2  # (_lay ends with the pad word and one word more)
    al = _aligner(True, ADAPT)
    try:
        for kk in (k, k - 5, 0):
            out = (torch.full((n,), -7, dtype=torch.int32, device="cuda:0"), torch.full((n,), -7, dtype=torch.int32, device="cuda:0"))
            with pytest.raises(wfa_amd._lib.WfaHipError) as e:
                al.score_tensors_packed(tens[0][:kk + SLACK], *tens[1:5], q_rc=tens[5], out=out)
            assert e.value.code == _lib.ERR_BAD_ARG
            assert bool((out[0] == -7).all()) and bool((out[1] == -7).all()), "the outputs were touched"
        bad = [a.copy() for a in pk]
        bad[1][3] = np.uint64((1 << 64) - 2)  # an offset that would wrap
        with pytest.raises(wfa_amd._lib.WfaHipError) as e:
            al.score_tensors_packed(*_to_device(bad, flags)[:5], q_rc=tens[5])
        assert e.value.code == _lib.ERR_BAD_ARG
        st, sc, _ = _call(al, tens)
        assert np.array_equal(st, want[0]) and np.array_equal(sc, want[1])
    finally:
        al.close()


# ---- 10. streams and caller-owned outputs
def test_side_stream_and_out_tensors():
    import torch
    qs, ts = _generated(115, 300, 300, 0.05)
    flags = (np.arange(len(qs)) % 2).astype(np.uint8)
    want = _oracle(qs, ts, True, ADAPT)
    src = _to_device(_buffers(qs, ts, flags), flags)
    n = len(qs)
    al = _aligner(True, ADAPT)
    try:
        s = torch.cuda.Stream(device="cuda:0")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):  # the inputs are produced on the side stream immediately before the call
            tens = [t.clone() for t in src]
            out = (torch.full((n + 64,), -7, dtype=torch.int32, device="cuda:0"), torch.full((n + 64,), -7, dtype=torch.int32, device="cuda:0"))
        r = al.score_tensors_packed(*tens[:5], q_rc=tens[5], out=out, stream=s)
        assert r[0] is out[0] and r[1] is out[1]
        torch.cuda.synchronize()
        assert np.array_equal(out[0].cpu().numpy()[:n], want[0]) and np.array_equal(out[1].cpu().numpy().view(np.uint32)[:n], want[1])
        assert bool((out[0][n:] == -7).all()) and bool((out[1][n:] == -7).all())
        for a, b in zip(tens, src):
            assert torch.equal(a, b), "an input tensor was written"
    finally:
        al.close()


# ---- 11. select_tensors against numpy.nonzero
@pytest.mark.parametrize("with_rc", [False, True])
def test_select_tensors(with_rc):
    import torch
    from wfa_amd import _lib
    rng = np.random.default_rng(116)
    al = _aligner(True, ADAPT)
    try:
        cases = [(0, "third"), (700, "none"), (700, "all")] + [(n, "third") for n in (SD_TILE - 1, SD_TILE, SD_TILE + 1, 3 * SD_TILE + 5)]
        for n, how in cases:
            status = np.where(rng.random(n) < 1 / 3, 0, rng.choice([1, 2, 4, 8], n)).astype(np.int32)
            if how != "third":
                status[:] = 8 if how == "none" else 0
            ins = [rng.integers(0, 1 << 62, n).astype(np.int64), rng.integers(0, 1 << 31, n).astype(np.int32),
                   rng.integers(0, 1 << 62, n).astype(np.int64), rng.integers(0, 1 << 31, n).astype(np.int32)]
            rc = rng.integers(0, 2, n).astype(np.uint8) if with_rc else None
            keep = np.nonzero(status == 0)[0]
            d = [_dev(status, np.int32)] + [_dev(a, a.dtype) for a in ins]
            d_rc = _dev(rc, np.uint8) if with_rc else None
            got = al.select_tensors(*d, q_rc=d_rc)
            assert len(got) == 6 and (got[5] is None) == (not with_rc)
            assert np.array_equal(got[0].cpu().numpy().view(np.uint32), keep.astype(np.uint32)), (n, how)
            for g, a, t in zip(got[1:5], ins, d[1:]):
                assert g.dtype == t.dtype and np.array_equal(g.cpu().numpy(), a[keep]), (n, how)
            if with_rc:
                assert np.array_equal(got[5].cpu().numpy(), rc[keep])
            if n == 0:
                continue
            # the raw entry: elements of the output arrays beyond the count keep their sentinels; d_idx may be NULL
            outs = [torch.full((n,), 0x5A, dtype=dt, device="cuda:0") for dt in (torch.int32, torch.int64, torch.int32, torch.int64, torch.int32)]
            outs.append(torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda:0") if with_rc else None)
            for idx_null in (False, True):
                cnt = C.c_uint64(99)
                torch.cuda.synchronize()
                ptr = lambda t: t.data_ptr() if t is not None else None
                r = _lib.lib().wfahip_select_pairs_device(al._ctx, d[0].data_ptr(), n, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                                          d[4].data_ptr(), ptr(d_rc), None if idx_null else outs[0].data_ptr(),
                                                          *[ptr(t) for t in outs[1:]], C.byref(cnt), None)
                assert r == 0 and cnt.value == len(keep)
                for o, a in zip(outs[1:5], ins):
                    h = o.cpu().numpy()
                    assert np.array_equal(h[:len(keep)], a[keep]) and (h[len(keep):] == 0x5A).all()
                h = outs[0].cpu().numpy()  # (written by the first of the two calls only)
                assert np.array_equal(h[:len(keep)].view(np.uint32), keep.astype(np.uint32)) and (h[len(keep):] == 0x5A).all()
                if with_rc:
                    h = outs[5].cpu().numpy()
                    assert np.array_equal(h[:len(keep)], rc[keep]) and (h[len(keep):] == 0x5A).all()
            for t, a in zip(d, [status] + ins):
                assert np.array_equal(t.cpu().numpy(), a), "an input tensor was written"
    finally:
        al.close()


# ---- 12. the chain, entirely in tensors
def test_chain_pack_score_select_align_cigar():
    """pack_tensors -> every pair listed twice (flag 0 and 1) -> score_tensors_packed(max_score = B) -> select_tensors ->
    align_tensors_packed(.., q_rc, max_score = B) -> cigar_tensors, against the host chain: score_arrays on the bytes of both strands,
    align_arrays on the survivors' bytes, cigar_text"""
    import torch
    import wfa_amd
    from test_align_packed_device_gpu import _as_batch
    from test_parity_gpu import assert_batch_equal
    n = 512
    qs, ts = _generated(117, n, 300, 0.05)
    flipped = (np.arange(n) % 2).astype(np.uint8)  # half of the queries lie reverse-complemented in the blob
    held = [_revcomp(q) if f else q for q, f in zip(qs, flipped)]
    al = _aligner(True, ADAPT)
    try:
        arrays = wfa_amd.make_blob(held, ts)
        blob, q_off, q_len, t_off, t_len = [_dev(a, dt) for a, dt in zip(arrays, (np.uint8, np.int64, np.int32, np.int64, np.int32))]
        # the host chain
        both_q = held + [_revcomp(q) for q in held]
        fst, fsc = al.score_arrays(*wfa_amd.make_blob(held, ts))
        bound = int(np.median(fsc[(flipped == 0) & (fst == 0)]))
        hst, hsc = al.score_arrays(*wfa_amd.make_blob(both_q, ts + ts), max_score=bound)
        keep = np.nonzero(hst == 0)[0]
        assert 0 < len(keep) < 2 * n
        want = al.align_arrays(*wfa_amd.make_blob([both_q[i] for i in keep], [(ts + ts)[i] for i in keep]), max_score=bound)
        wt, wo = wfa_amd.cigar_text(want)
        # the chain in tensors
        packed, q_woff, t_woff = al.pack_tensors(blob, q_off, q_len, t_off, t_len)
        twice = lambda t: torch.cat([t, t])
        rc = torch.cat([torch.zeros(n, dtype=torch.uint8, device="cuda:0"), torch.ones(n, dtype=torch.uint8, device="cuda:0")])
        cand = (twice(q_woff), twice(q_len), twice(t_woff), twice(t_len))
        st, sc = al.score_tensors_packed(packed, *cand, q_rc=rc, max_score=bound)
        assert np.array_equal(st.cpu().numpy(), hst) and np.array_equal(sc.cpu().numpy().view(np.uint32), hsc)
        idx, s_qw, s_ql, s_tw, s_tl, s_rc = al.select_tensors(st, *cand, q_rc=rc)
        assert np.array_equal(idx.cpu().numpy().view(np.uint32), keep.astype(np.uint32))
        rec, ops = al.align_tensors_packed(packed, s_qw, s_ql, s_tw, s_tl, q_rc=s_rc, max_score=bound)
        text, off = al.cigar_tensors(rec, ops)
        assert_batch_equal(_as_batch(rec, ops), want, "the chain's records")
        assert (want.status == 0).all()
        assert np.array_equal(off.cpu().numpy().view(np.uint64), wo) and text.cpu().numpy().tobytes() == wt.tobytes()
    finally:
        al.close()
