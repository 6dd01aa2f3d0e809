"""GPU: wfahip_score_batch_device (Aligner.score_tensors) on a batch resident in HBM returns, pair for pair, the status and score
of the oracle and of wfahip_score_batch on the same bytes -- and routes as it does (n_retried_pairs, arena_bytes, kernel kind):
global and semi-global, wf-adaptive on and off, every penalty shape, any bytes, long pairs through the device-side plan / pack /
list kernels (their buffer word for word the host's), max_score, streams, caller-owned outputs, chunks, and the bounds check."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ADAPT = (10, 50, 1)
MODES = [(g, a) for g in (True, False) for a in (ADAPT, None)]
PAD = 64  # bytes behind the sequences in a device blob (the kernels' aligned loads at the tail stay inside the allocation)


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
    w = O.align_batch(O.make_params(*pen, global_alignment=glob, adaptive=adaptive), *arrays, n_threads=16, want_ops=False)
    return w.status, np.where(w.status == 0, w.score, 0).astype(np.uint32)


def _to_device(arrays):
    import torch
    blob, q_off, q_len, t_off, t_len = arrays
    blob = np.concatenate([np.ascontiguousarray(blob, np.uint8), np.zeros(PAD, np.uint8)])
    host = (blob, np.ascontiguousarray(q_off, np.uint64).view(np.int64), np.ascontiguousarray(q_len, np.uint32).view(np.int32),
            np.ascontiguousarray(t_off, np.uint64).view(np.int64), np.ascontiguousarray(t_len, np.uint32).view(np.int32))
    return tuple(torch.from_numpy(a.copy()).to("cuda:0") for a in host)


def _np(status, score, n=None):
    st, sc = status.cpu().numpy(), score.cpu().numpy().view(np.uint32)
    return (st, sc) if n is None else (st[:n], sc[:n])


def _tm(al):
    t = al.last_timing()
    return t.main_kernel_kind, t.n_retried_pairs, t.arena_bytes


def _both(al, arrays, glob=True, adaptive=ADAPT, pen=(4, 6, 2), max_score=0, oracle=True, label=""):
    """The device entry against the host entry (status, score, kind, retried, arena) and against the oracle; returns the
    device entry's (status, score, (kind, retried, arena))."""
    hst, hsc = al.score_arrays(*arrays, max_score=max_score)
    ht = _tm(al)
    dst, dsc = _np(*al.score_tensors(*_to_device(arrays), max_score=max_score))
    dt = _tm(al)
    print(f"{label} n={len(hst)} host(kind, retried, arena)={ht} device={dt} mismatches vs host: status {(hst != dst).sum()} score {(hsc != dsc).sum()}")
    assert np.array_equal(dst, hst) and np.array_equal(dsc, hsc)
    assert dt == ht
    if oracle and max_score == 0:
        wst, wsc = _oracle(arrays, glob, adaptive, pen)
        assert np.array_equal(dst, wst) and np.array_equal(dsc, wsc)
    return dst, dsc, dt


def _golden_pairs():
    ka = json.load(open(os.path.join(GOLDEN, "known_answers.json")))["vectors"]
    ref = json.load(open(os.path.join(GOLDEN, "ref_test_pairs.json")))
    return [(v["q"].encode(), v["t"].encode()) for v in ka] + [(p["q"].encode(), p["t"].encode()) for p in ref]


def _rand(rng, n):
    return bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))


def _mutate(rng, s, rate):
    out = bytearray()
    for c in s:
        r = rng.random()
        if r < rate / 3:
            out.append(b"ACGT"[rng.integers(4)])
        elif r < 2 * rate / 3:
            continue
        elif r < rate:
            out += bytes([c, b"ACGT"[rng.integers(4)]])
        else:
            out.append(c)
    return bytes(out)


def _tight_blob(qs, ts, lead=None):
    """Sequences laid end to end, no alignment; lead[i] filler bytes in front of pair i's query."""
    parts, q_off, t_off, pos = [], [], [], 0
    for i, (q, t) in enumerate(zip(qs, ts)):
        fill = b"#" * (lead[i] if lead else 0)
        parts.append(fill), parts.append(q), parts.append(t)
        q_off.append(pos + len(fill)), t_off.append(pos + len(fill) + len(q))
        pos += len(fill) + len(q) + len(t)
    blob = np.frombuffer(b"".join(parts) or b"\0", np.uint8).copy()
    return (blob, np.array(q_off, np.uint64), np.array([len(q) for q in qs], np.uint32), np.array(t_off, np.uint64),
            np.array([len(t) for t in ts], np.uint32))


# ---- 1. golden pairs and generated batches
@pytest.mark.parametrize("glob,adaptive", MODES)
def test_golden_pairs(glob, adaptive):
    import wfa_amd
    _both(_aligner(glob, adaptive), wfa_amd.make_blob(*zip(*_golden_pairs())), glob, adaptive, label="golden")


@pytest.mark.parametrize("adaptive", [ADAPT, None])
@pytest.mark.parametrize("err", [0.05, 0.10, 0.20])
def test_generated_global(adaptive, err):
    import wfa_amd
    al = _aligner(True, adaptive)
    # (1 kbp without wf-adaptive: 512 pairs, the oracle's rows stay n + m wide)
    _, _, t = _both(al, wfa_amd.generate_pairs(seed=11, n_pairs=2048 if adaptive else 512, length=1000, error_rate=err), True, adaptive,
                    label=f"1kbp {err}")
    if adaptive and err == 0.05:
        assert t == (19, 0, 0)  # (KERNELS.md 4g: no pair of this class leaves the score kernel)
    _both(al, wfa_amd.generate_pairs(seed=12, n_pairs=4096, length=150, error_rate=err), True, adaptive, label=f"150bp {err}")


# ---- 2. penalty shapes
@pytest.mark.parametrize("pen", [(4, 6, 2), (2, 4, 2), (1, 1, 1), (4, 4, 2), (4, 2, 2), (6, 4, 2), (5, 7, 3)])
@pytest.mark.parametrize("glob", [True, False])
def test_penalty_shapes(pen, glob):
    import wfa_amd
    arrays = wfa_amd.generate_pairs(seed=8, n_pairs=512, length=300, error_rate=0.05)
    _, _, t = _both(_aligner(glob, ADAPT, pen), arrays, glob, ADAPT, pen, label=f"pen {pen}")
    if pen == (5, 7, 3):  # e / g = 3: no instance -- everything through the redo kernel and the full path
        assert t[1] == 512


# ---- 3. a mixed batch
@pytest.mark.parametrize("glob,adaptive", MODES)
def test_mixed_batch(glob, adaptive):
    rng = np.random.default_rng(3)
    qs, ts = [], []
    for i in range(240):
        n = int(rng.integers(1, 900))
        q = _rand(rng, n)
        t = _mutate(rng, q, 0.05) or b"A"
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
    wide = _rand(rng, 1500)
    qs.append(wide), ts.append(_mutate(rng, wide, 0.20))  # without wf-adaptive its band outgrows the kernels' 248 diagonals
    semi = _rand(rng, 2300)
    qs.append(semi[300:2000]), ts.append(_mutate(rng, semi, 0.03))  # a 2 300-base target: beyond the wide kernel's 2 047
    arrays = list(_tight_blob(qs, ts))
    # forty pairs sharing ONE target offset, and a length over WFAHIP_MAX_SEQ_LEN at offset 0 (never read)
    shared = _rand(rng, 700)
    extra_q = [_mutate(rng, shared, 0.04) for _ in range(40)]
    base = len(arrays[0])
    blob2, q_off2, q_len2, _, _ = _tight_blob(extra_q, [b""] * 40)
    arrays[0] = np.concatenate([arrays[0], blob2, np.frombuffer(shared, np.uint8)])
    arrays[1] = np.concatenate([arrays[1], q_off2 + np.uint64(base), np.array([0, 0], np.uint64)])
    arrays[2] = np.concatenate([arrays[2], q_len2, np.array([1 << 29, 5], np.uint32)])
    arrays[3] = np.concatenate([arrays[3], np.full(40, base + len(blob2), np.uint64), np.array([0, 0], np.uint64)])
    arrays[4] = np.concatenate([arrays[4], np.full(40, 700, np.uint32), np.array([5, 1 << 29], np.uint32)])
    st, _, _ = _both(_aligner(glob, adaptive), tuple(arrays), glob, adaptive, label="mixed")
    assert (st[1:240:6] == 1).all() and (st[2:240:6] == 1).all() and (st[-2:] == 2).all()


# ---- 4. long global pairs
def _long_pairs(seed, n, length=3000, rate=0.03):
    rng = np.random.default_rng(seed)
    qs = [_rand(rng, length) for _ in range(n)]
    return qs, [_mutate(rng, q, rate) for q in qs]


def _device_list(al):
    from wfa_amd import _lib as L
    w, t, nw, nl = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.c_uint64(), C.c_uint64()
    L.check(L.lib().wfahip_debug_score_device_list(al._ctx, C.byref(w), C.byref(nw), C.byref(t), C.byref(nl)))
    words = np.ctypeslib.as_array(w, shape=(nw.value,)).copy() if nw.value else np.zeros(0, np.uint32)
    table = np.ctypeslib.as_array(t, shape=(nl.value * 8,)).copy() if nl.value else np.zeros(0, np.uint32)
    L.lib().wfahip_free(w), L.lib().wfahip_free(t)
    return words, table


def _host_list(arrays):
    from wfa_amd import _lib as L
    blob, q_off, q_len, t_off, t_len = [np.ascontiguousarray(a) for a in arrays]
    w, t, nw, nl = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.c_uint64(), C.c_uint64()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    L.check(L.lib().wfahip_debug_score_long_list(vp(blob), vp(q_off), vp(q_len), vp(t_off), vp(t_len), len(q_len), C.byref(w), C.byref(nw),
                                                 C.byref(t), C.byref(nl)))
    words = np.ctypeslib.as_array(w, shape=(nw.value,)).copy() if nw.value else np.zeros(0, np.uint32)
    table = np.ctypeslib.as_array(t, shape=(nl.value * 8,)).copy() if nl.value else np.zeros(0, np.uint32)
    L.lib().wfahip_free(w), L.lib().wfahip_free(t)
    return words, table


def test_long_pairs_at_the_default_gate():
    import wfa_amd
    qs, ts = _long_pairs(51, 64)
    _, _, t = _both(_aligner(), wfa_amd.make_blob(qs, ts), label="64 x 3 kbp")
    assert t == (23, 0, 0)
    # one pair fewer: under the gate, the full path -- kind and counts as the host entry's (asserted in _both)
    _, _, t = _both(_aligner(), wfa_amd.make_blob(qs[:63], ts[:63]), label="63 x 3 kbp")
    assert t[1] == 63 and t[0] != 23 and t[2] > 0


def test_long_pairs_packed_on_the_device():
    rng = np.random.default_rng(52)
    qs, ts, lead = [], [], []
    for i, ln in enumerate([2046, 2047, 2048, 2049] * 2):  # around SCORE_MAX_LEN, on either side
        a = _rand(rng, ln)
        b = _mutate(rng, a, 0.02)
        qs.append(a if i < 4 else b), ts.append(b if i < 4 else a)
    for i in range(40):  # lengths of every residue modulo 16, laid end to end: sequence starts at every byte offset
        a = _rand(rng, 2100 + 37 * i)
        qs.append(a), ts.append(_mutate(rng, a, 0.03))
    qs.append(_rand(rng, 500)), ts.append(qs[-1])  # a short pair among them
    n_tail = _rand(rng, 2500)
    qs.append(n_tail), ts.append(n_tail[:-1] + b"N")  # listed by its lengths, an N in its last base: the full path
    lead = [i % 16 for i in range(len(qs))]
    arrays = _tight_blob(qs, ts, lead)
    starts = {int(o) % 16 for o in arrays[1]} | {int(o) % 16 for o in arrays[3]}
    assert starts == set(range(16))
    al = _aligner(long_min=1)
    st, sc, t = _both(al, arrays, label="long, gate 1")
    assert t[0] == 23 and t[1] >= 1
    assert st[-1] == 0 and sc[-1] == 4  # (one mismatch)
    dw, dt = _device_list(al)  # (of the device call, the last score call on al)
    hw, ht = _host_list(arrays)
    print("packed words", len(hw), "listed", len(ht) // 8, "word mismatches", int((dw != hw).sum()) if len(dw) == len(hw) else "length")
    assert len(hw) > 0 and np.array_equal(dw, hw) and np.array_equal(dt, ht)
    assert len(ht) // 8 == sum(1 for q, t_ in zip(qs, ts) if max(len(q), len(t_)) > 2047) - 1
    # a small window: the same results
    st2, sc2, t2 = _both(_aligner(long_min=1, window=16), arrays, oracle=False, label="long, window 16")
    assert np.array_equal(st2, st) and np.array_equal(sc2, sc) and t2 == t


# ---- 5. max_score
@pytest.mark.parametrize("glob", [True, False])
def test_max_score(glob):
    import wfa_amd
    g = wfa_amd.generate_pairs(seed=9, n_pairs=1024, length=1000, error_rate=0.10)
    qs = [bytes(g[0][int(o):int(o) + int(n)]) for o, n in zip(g[1], g[2])]
    ts = [bytes(g[0][int(o):int(o) + int(n)]) for o, n in zip(g[3], g[4])]
    lq, lt = _long_pairs(53, 32, 3000, 0.01)  # (scores on either side of the short pairs' median)
    lq2, lt2 = _long_pairs(54, 32, 3000, 0.06)
    lq, lt = lq + lq2, lt + lt2
    for i in range(0, 1024, 8):  # bytes outside ACGT: pairs of the full path (both lowercase: the scores stay those of the letters)
        qs[i], ts[i] = qs[i].lower(), ts[i].lower()
    arrays = wfa_amd.make_blob(qs + lq, ts + lt)
    al = _aligner(glob)
    _, sc, _ = _both(al, arrays, glob, label="max_score 0")
    bound = int(np.median(sc))
    st, sc2, _ = _both(al, arrays, glob, max_score=bound, label=f"max_score {bound}")
    over = sc > bound
    assert over[:1024:8].any() and (~over)[:1024:8].any() and over[1024:].any() and (~over)[1024:].any()
    assert (st[over] == 8).all() and (sc2[over] == 0).all() and (st[~over] == 0).all() and np.array_equal(sc2[~over], sc[~over])


# ---- 6. device-born input
def test_device_generated_input():
    import wfa_amd
    al = _aligner()
    tens = wfa_amd.generate_pairs_device(al, seed=21, n_pairs=4096, length=400, error_rate=0.05)
    st, sc = _np(*al.score_tensors(*tens))
    wst, wsc = _oracle(wfa_amd.generate_pairs(seed=21, n_pairs=4096, length=400, error_rate=0.05))
    assert np.array_equal(st, wst) and np.array_equal(sc, wsc)


# ---- 7. stream and buffers
def test_stream_inputs_and_out_tensors():
    import torch
    import wfa_amd
    arrays = wfa_amd.generate_pairs(seed=22, n_pairs=3000, length=300, error_rate=0.05)
    n = 3000
    wst, wsc = _oracle(arrays)
    al = _aligner()
    staged = [t.clone() for t in _to_device(arrays)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device="cuda:0")
    status = torch.full((n + 64,), -7, dtype=torch.int32, device="cuda:0")
    score = torch.full((n + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        tens = [torch.empty_like(t) for t in staged]
        for dst, src in zip(tens, staged):  # the inputs are produced on s, immediately before the call
            dst.copy_(src + 0, non_blocking=True)
        before = [t.clone() for t in tens]
        got = al.score_tensors(*tens, out=(status, score), stream=s)
    assert got[0] is status and got[1] is score
    st, sc = _np(status, score)
    assert np.array_equal(st[:n], wst) and np.array_equal(sc[:n], wsc)
    assert (st[n:] == -7).all() and (sc[n:] == 0x5A5A5A5A).all()
    for a, b in zip(tens, before):
        assert torch.equal(a, b)


# ---- 8. chunks
def test_two_chunks_of_the_wide_kernel():
    import wfa_amd
    n = (1 << 18) + 5
    arrays = wfa_amd.generate_pairs(seed=23, n_pairs=n, length=40, error_rate=0.05)
    _, _, t = _both(_aligner(False), arrays, False, oracle=False, label="2^18 + 5 semi-global")
    assert t[0] == 20


# ---- 9. bounds
def test_offsets_outside_the_blob_are_refused():
    import torch
    import wfa_amd
    arrays = wfa_amd.generate_pairs(seed=24, n_pairs=64, length=200, error_rate=0.05)
    tens = _to_device(arrays)
    al = _aligner()
    half = tens[0].numel() // 2
    assert int(arrays[3][-1]) + int(arrays[4][-1]) > half  # (the last target lies in the upper half of the allocation)
    status = torch.full((64,), -7, dtype=torch.int32, device="cuda:0")
    score = torch.full((64,), 77, dtype=torch.int32, device="cuda:0")
    with pytest.raises(wfa_amd._lib.WfaHipError) as e:
        al.score_tensors(tens[0][:half], *tens[1:], out=(status, score))  # (a view: blob_bytes = half of the real allocation)
    assert e.value.code == wfa_amd._lib.ERR_BAD_ARG
    assert (status == -7).all() and (score == 77).all()
    st, sc = _np(*al.score_tensors(*tens, out=(status, score)))  # the next call on the context works
    wst, wsc = _oracle(arrays)
    assert np.array_equal(st, wst) and np.array_equal(sc, wsc)
