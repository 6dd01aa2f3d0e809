"""GPU: CIGAR text rendered on the device (include/wfa_hip.h: wfahip_cigar_text_device, wfahip_align_batch_text; Aligner.cigar_tensors,
align_tensors, align_arrays_text).  The three kernels on synthetic records and ops (tests/cigar_cases.py: digit boundaries, the trim
cases, the seams of the 64-op rounds and of the scan blocks, ops out of pair order with junk between them) against the Python
restatement of AlignmentResult.CIGAR, byte for byte, with everything behind the text still poisoned and the inputs unchanged; the
capacity and range errors; a caller-owned stream; and end to end against the oracle's own strings."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cigar_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu
ADAPT = (10, 50, 1)
PAD = 64      # bytes behind the sequences in a device blob (the kernels' aligned loads at the tail stay inside the allocation)
POISON = 0xA5
SCAN_BLOCK_PAIRS = 4096  # wfa_cigar.hip: CIG_SCAN_BLOCK * CIG_SCAN_ITEMS


@pytest.fixture(scope="module")
def al(built):
    import wfa_amd
    a = wfa_amd.New(wfa_amd.DefaultPenalties, wfa_amd.Options(GlobalAlignment=True), device=0)
    assert a.AdaptiveReduction(wfa_amd.AdaptiveReductionOption(*ADAPT)) is None
    yield a
    a.close()


@pytest.fixture(scope="module")
def al_semi(built):
    import wfa_amd
    a = wfa_amd.New(wfa_amd.DefaultPenalties, wfa_amd.Options(GlobalAlignment=False), device=0)
    assert a.AdaptiveReduction(wfa_amd.AdaptiveReductionOption(*ADAPT)) is None
    yield a
    a.close()


@functools.lru_cache(maxsize=None)
def _synthetic(n):
    """n cases -- the multi-round pairs first, so that the smallest batches hold them -- laid out, with both expected texts"""
    seam, base = K.seam_cases(), K.base_cases()
    pool = [seam[9], base[0], seam[10], seam[4], base[8]] + seam[:4] + seam[5:9] + seam[11:] + base[1:8] + base[9:]
    cases = [pool[i % len(pool)] for i in range(n)]
    status, ops_off, ops_len, ops = K.lay_out(cases, seed=100 + n)
    return K.records(status, ops_off, ops_len), ops, K.expected(cases, 0), K.expected(cases, 1)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy((a.view(view) if view else a).copy()).to("cuda:0")


def _raw(al, rec, ops, only, text, text_cap, off, stream=None, ops_cap=None):
    """the C entry itself: (return code, *text_needed)"""
    import torch
    from wfa_amd import _lib
    torch.cuda.synchronize()  # (the fills of the test ran on torch's stream; stream=None is the context's own)
    need = C.c_uint64(12345)
    rc = _lib.lib().wfahip_cigar_text_device(al._ctx, rec.data_ptr(), ops.data_ptr(), ops.numel() if ops_cap is None else ops_cap,
                                             rec.shape[0], only, text.data_ptr() if text is not None else None, text_cap,
                                             off.data_ptr(), C.byref(need), stream)
    return rc, need.value


@pytest.mark.parametrize("n", [1, 3, 4, 5, SCAN_BLOCK_PAIRS + 1])
@pytest.mark.parametrize("only", [0, 1])
def test_synthetic_records(al, only, n):
    import torch
    rec_h, ops_h, *want = _synthetic(n)
    want_text, want_off = want[only]
    rec, ops = _dev(rec_h), _dev(ops_h)
    rec0, ops0 = rec.clone(), ops.clone()
    total = len(want_text)
    text = torch.full((total + 257,), POISON, dtype=torch.uint8, device="cuda:0")  # larger than needed, poisoned
    off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda:0")
    t2, o2 = al.cigar_tensors(rec, ops, only_aligned=bool(only), out=(text, off))
    assert t2 is text and o2 is off
    got_text, got_off = text.cpu().numpy(), off.cpu().numpy().view(np.uint64)
    assert got_off[0] == 0 and got_off[n] == total
    assert np.array_equal(got_off, want_off)
    bad = np.flatnonzero(got_text[:total] != want_text)
    assert bad.size == 0, f"first differing byte {bad[:1]} of {total}"
    assert (got_text[total:] == POISON).all()                      # nothing at or beyond d_text_off[n] is written
    assert torch.equal(rec, rec0) and torch.equal(ops, ops0)        # the inputs are only read
    # out=None: one sizing call, then exactly the text
    t3, o3 = al.cigar_tensors(rec, ops, only_aligned=bool(only))
    assert t3.numel() == total and t3.cpu().numpy().tobytes() == want_text.tobytes()
    assert np.array_equal(o3.cpu().numpy().view(np.uint64), want_off)


def test_capacity_errors_and_sizing_call(al):
    import torch
    from wfa_amd import _lib
    rec_h, ops_h, (want_text, want_off), _ = _synthetic(5)
    rec, ops = _dev(rec_h), _dev(ops_h)
    total, n = len(want_text), 5
    text = torch.full((total + 64,), POISON, dtype=torch.uint8, device="cuda:0")
    off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda:0")
    rc, need = _raw(al, rec, ops, 0, text, total - 1, off)
    assert rc == _lib.ERR_OOM and need == total
    assert (text.cpu().numpy() == POISON).all()                                    # d_text untouched
    assert np.array_equal(off.cpu().numpy().view(np.uint64), want_off)             # d_text_off filled
    rc, need = _raw(al, rec, ops, 0, text, total, off)                             # exactly the total: fits
    assert rc == 0 and need == total
    got = text.cpu().numpy()
    assert got[:total].tobytes() == want_text.tobytes() and (got[total:] == POISON).all()
    off.fill_(-1)
    rc, need = _raw(al, rec, ops, 0, None, 0, off)                                 # the sizing call
    assert rc == _lib.ERR_OOM and need == total and np.array_equal(off.cpu().numpy().view(np.uint64), want_off)
    # no pairs: d_text_off[0] = 0 and nothing else
    off.fill_(-1)
    rc, need = _raw(al, rec[:0], ops, 0, text, total, off)
    assert rc == 0 and need == 0 and off.cpu().numpy().tolist() == [0] + [-1] * n


@pytest.mark.parametrize("where", ["one_past_the_end", "off_2_63", "len_over_cap"])
def test_op_range_outside_the_buffer(al, where):
    import torch
    from wfa_amd import _lib
    rec_h, ops_h, _, _ = _synthetic(5)
    rec_h = rec_h.copy()
    cap = len(ops_h)
    ln = 3
    o = {"one_past_the_end": cap - ln + 1, "off_2_63": 1 << 63, "len_over_cap": 0}[where]
    if where == "len_over_cap":
        ln = cap + 1
    rec_h[2, 0], rec_h[2, 10], rec_h[2, 11], rec_h[2, 12] = 0, ln, o & 0xFFFFFFFF, o >> 32
    rec, ops = _dev(rec_h), _dev(ops_h)
    text = torch.full((8192,), POISON, dtype=torch.uint8, device="cuda:0")
    off = torch.zeros(6, dtype=torch.int64, device="cuda:0")
    rc, _need = _raw(al, rec, ops, 0, text, text.numel(), off)
    assert rc == _lib.ERR_BAD_ARG
    assert (text.cpu().numpy() == POISON).all()
    # the same record fits once the range ends exactly at the capacity
    if where == "one_past_the_end":
        rec_h[2, 11] = cap - ln
        rc, _need = _raw(al, _dev(rec_h), ops, 0, text, text.numel(), off)
        assert rc == 0


def test_caller_owned_stream(al):
    import torch
    rec_h, ops_h, _, (want_text, want_off) = _synthetic(SCAN_BLOCK_PAIRS + 1)
    rec, ops = _dev(rec_h), _dev(ops_h)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(s):
        text, off = al.cigar_tensors(rec, ops, only_aligned=True, stream=s)
    assert text.cpu().numpy().tobytes() == want_text.tobytes()
    assert np.array_equal(off.cpu().numpy().view(np.uint64), want_off)


def _seqs(arrays):
    blob, q_off, q_len, t_off, t_len = arrays
    b = blob.tobytes()
    qs = [b[int(o):int(o) + int(n)] for o, n in zip(q_off, q_len)]
    ts = [b[int(o):int(o) + int(n)] for o, n in zip(t_off, t_len)]
    return qs, ts


@functools.lru_cache(maxsize=None)
def _batch(glob):
    """about 300 pairs and the oracle's strings for them.  Global: 150 bases @2 %, an empty pair, a pair with an N, A against C.
    Semi-global: 300 bases @5 % with the target overhanging on both sides."""
    import wfa_amd
    rng = np.random.default_rng(77)
    if glob:
        qs, ts = _seqs(wfa_amd.generate_pairs(seed=21, n_pairs=300, length=150, error_rate=0.02))
        qs += [b"", b"ACGTNACGTTGCA", b"A"]
        ts += [b"ACGT", b"ACGTAACGTTGCA", b"C"]
    else:
        qs, ts = _seqs(wfa_amd.generate_pairs(seed=22, n_pairs=300, length=300, error_rate=0.05))
        rnd = lambda k: bytes(rng.choice(list(b"ACGT"), k).astype(np.uint8))
        ts = [rnd(int(rng.integers(1, 60))) + t + rnd(int(rng.integers(1, 60))) for t in ts]
    arrays = wfa_amd.make_blob(qs, ts)
    w = O.align_batch(O.make_params(global_alignment=glob, adaptive=ADAPT), *arrays, n_threads=8)
    full, trimmed = [], []
    for i in range(len(qs)):
        r = O.Result(status=int(w.status[i]), ops=[int(x) for x in w.pair_ops(i)] if w.status[i] == 0 else [])
        full.append(r.cigar), trimmed.append(r.cigar_trimmed())
    return arrays, w, full, trimmed


def _to_device(arrays):
    blob, q_off, q_len, t_off, t_len = arrays
    return (_dev(np.concatenate([np.ascontiguousarray(blob, np.uint8), np.zeros(PAD, np.uint8)])), _dev(np.asarray(q_off, np.uint64)),
            _dev(np.asarray(q_len, np.uint32)), _dev(np.asarray(t_off, np.uint64)), _dev(np.asarray(t_len, np.uint32)))


def _strings(text, off):
    t, o = text.cpu().numpy().tobytes(), off.cpu().numpy()
    return [t[int(o[i]):int(o[i + 1])].decode("latin-1") for i in range(len(o) - 1)]


@pytest.mark.parametrize("glob", [True, False])
def test_end_to_end_against_the_oracle(al, al_semi, glob):
    a = al if glob else al_semi
    arrays, w, full, trimmed = _batch(glob)
    rec, ops = a.align_tensors(*_to_device(arrays))
    st = rec.cpu().numpy()[:, 0]
    assert np.array_equal(st, w.status)
    assert _strings(*a.cigar_tensors(rec, ops)) == full
    assert _strings(*a.cigar_tensors(rec, ops, only_aligned=True)) == trimmed
    if glob:
        assert full[-3:] == ["", full[-2], "1X"] and trimmed[-1] == "" and (w.status[-3:] == [1, 0, 0]).all()
    else:
        assert sum(f != t for f, t in zip(full, trimmed)) > 100  # the overhangs are trimmed away


def test_bounded_records_render_empty(al):
    arrays, w, full, trimmed = _batch(True)
    bound = int(np.median(w.score[w.status == 0]))
    rec, ops = al.align_tensors(*_to_device(arrays), max_score=bound)
    st = rec.cpu().numpy()[:, 0]
    over = (w.status == 0) & (w.score > bound)
    assert over.sum() > 20 and (~over).sum() > 20
    assert (st[over] == 8).all() and np.array_equal(st[~over], w.status[~over])
    assert _strings(*al.cigar_tensors(rec, ops)) == ["" if o else f for o, f in zip(over, full)]
    assert _strings(*al.cigar_tensors(rec, ops, only_aligned=True)) == ["" if o else t for o, t in zip(over, trimmed)]


def _check_text_entry(a, arrays, only):
    import wfa_amd
    want = a.align_arrays(*arrays)
    got, text, off = a.align_arrays_text(*arrays, only_aligned=only)
    n = len(want.status)
    for f in ("status", "score", "tbegin", "tend", "qbegin", "qend", "align_len", "matches", "gaps", "gap_regions", "ops_len"):
        assert np.array_equal(getattr(got, f), getattr(want, f)), f
    assert got.ops.size == 0 and not got.ops_off.any() and got.ops_off.shape == (n,)
    strings = [want.result(i).CIGAR(only) if want.status[i] == 0 else "" for i in range(n)]
    assert text.dtype == np.uint8 and off.dtype == np.uint64 and off.shape == (n + 1,) and off[0] == 0 and off[n] == len(text)
    assert text.tobytes().decode("latin-1") == "".join(strings)
    assert [int(x) for x in np.diff(off.astype(np.int64))] == [len(s) for s in strings]
    # ... and the host renderer over the ops that entry downloads gives the same bytes
    t2, o2 = wfa_amd.cigar_text(want, only_aligned=only, n_threads=4)
    assert np.array_equal(t2, text) and np.array_equal(o2, off)
    return strings


@pytest.mark.parametrize("glob", [True, False])
def test_align_arrays_text(al, al_semi, glob):
    a = al if glob else al_semi
    arrays, w, full, trimmed = _batch(glob)
    assert _check_text_entry(a, arrays, False) == full
    assert _check_text_entry(a, arrays, True) == trimmed


def test_align_arrays_text_known_answers_and_buffer_reuse(al, al_semi, known_answers):
    import wfa_amd
    for a, mode in ((al, "global"), (al_semi, "semi-global")):
        kas = [k for k in known_answers["vectors"] if k["mode"] == mode and list(k.get("adaptive") or []) == list(ADAPT)]
        if not kas:
            continue
        arrays = wfa_amd.make_blob([k["q"].encode() for k in kas], [k["t"].encode() for k in kas])
        strings = _check_text_entry(a, arrays, False)
        for k, s in zip(kas, strings):
            if k.get("cigar_exact"):
                assert s == k["cigar"], k["id"]
    assert any(k.get("cigar_exact") and k["mode"] == "global" and list(k.get("adaptive") or []) == list(ADAPT) for k in known_answers["vectors"])
    # the context's buffers reused: a smaller batch, then a larger one, then the first again
    arrays, w, full, trimmed = _batch(True)
    blob, q_off, q_len, t_off, t_len = arrays
    small = (blob, q_off[:7], q_len[:7], t_off[:7], t_len[:7])
    qs, ts = _seqs(arrays)
    large = wfa_amd.make_blob(qs + qs[:200], ts + ts[:200])
    assert _check_text_entry(al, small, False) == full[:7]
    assert _check_text_entry(al, large, True) == trimmed + trimmed[:200]
    assert _check_text_entry(al, arrays, False) == full
    # no pairs at all
    z64, z32 = np.zeros(0, np.uint64), np.zeros(0, np.uint32)
    got, text, off = al.align_arrays_text(np.zeros(1, np.uint8), z64, z32, z64, z32)
    assert got.status.size == 0 and text.size == 0 and off.tolist() == [0]
